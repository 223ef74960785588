"""CPU: lyric alignment on the native DiT (ace355.align, NativeDitMixin.get_lyric_timestamp / get_lyric_score) - the pair list, the
reference's bf16 rows, the handlers' layout, the mixin's payloads and fallbacks on a stub host, and the tiny G18 case against the oracle."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import ace355
from ace355 import align
from ace355.backend import NativeDitMixin

from _xattn_capture import G18_ORACLE_BOUND, capture_cross, checksum, g18_inputs, g18_score_rows, handler_layout

FULL = ace355.DitConfig()
TINY = dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, head_dim=128)


# ------------------------------------------------------------------------------------------------ pairs
def test_default_pairs_match_the_reference_handler():
    assert align.DEFAULT_LAYERS_HEADS == {2: [6], 3: [10, 11], 4: [3], 5: [8, 9], 6: [8]}   # acestep/handler.py:129
    assert align.pairs(align.DEFAULT_LAYERS_HEADS, FULL) == [(2, 6), (3, 10), (3, 11), (4, 3), (5, 8), (5, 9), (6, 8)]


def test_pairs_sort_and_dedup():
    assert align.pairs({5: [9, 8, 9], 0: [1, 0], 3: (2,)}, FULL) == [(0, 0), (0, 1), (3, 2), (5, 8), (5, 9)]


@pytest.mark.parametrize("bad", [{}, {24: [0]}, {-1: [0]}, {2: [16]}, {2: [-1]}, {"2": [6]}, {2: ["6"]}, {2: [6.0]}, {2: 6}, {2: []},
                                 {True: [0]}])
def test_pairs_refuse(bad):
    with pytest.raises(ValueError):
        align.pairs(bad, FULL)


# ------------------------------------------------------------------------------------------------ rows
def _pred_noise(B, T=9):
    g = torch.Generator().manual_seed(3)
    return torch.randn(B, T, 64, generator=g).to(torch.bfloat16), torch.randn(B, T, 64, generator=g).to(torch.bfloat16)


@pytest.mark.parametrize("steps", [8, 3, 1])
def test_timestamp_rows_are_the_reference_bf16_expressions(steps):
    pred, noise = _pred_noise(2)
    x, t = align.alignment_rows(pred, noise, steps, "timestamp")
    tl = 1.0 / steps   # H/lyric_timestamp.py:71-75, in bf16 tensor arithmetic
    assert x.dtype == torch.bfloat16 and torch.equal(x, tl * noise + (1.0 - tl) * pred)
    assert torch.equal(t, torch.tensor([tl, tl], dtype=torch.bfloat16))


def test_score_rows_are_the_reference_bf16_expressions():
    pred, noise = _pred_noise(2)
    x, t = align.alignment_rows(pred, noise, 8, "score")
    tl = 1.0 / 8   # H/lyric_score.py:70-80
    assert torch.equal(x, torch.cat([noise, tl * noise + (1.0 - tl) * pred], 0))
    assert torch.equal(t, torch.cat([torch.tensor([1.0, 1.0], dtype=torch.bfloat16), torch.tensor([tl, tl], dtype=torch.bfloat16)]))
    x3, t3 = align.alignment_rows(pred[:1], noise[:1], 3, "score")
    assert float(t3[1]) != 1.0 / 3 and float(t3[1]) == float(torch.tensor(1.0 / 3, dtype=torch.bfloat16))   # the reference's t rounding


@pytest.mark.parametrize("steps", [0, -1, 2.0, "8", None])
def test_rows_refuse_bad_steps(steps):
    pred, noise = _pred_noise(1)
    with pytest.raises(ValueError, match=f"inference_steps must be a positive non-zero integer, got {steps!r}"):
        align.alignment_rows(pred, noise, steps, "timestamp")


def test_noise_like_follows_sample_noise_like():
    pred = torch.zeros(2, 5, 64, dtype=torch.bfloat16)
    g = torch.Generator(device="cpu").manual_seed(42)
    assert torch.equal(align.noise_like(pred, 42), torch.randn(pred.shape, generator=g, dtype=torch.bfloat16))
    assert align.noise_like(pred, None).shape == pred.shape and align.noise_like(pred, None).dtype == torch.bfloat16


# ------------------------------------------------------------------------------------------------ stack
def _maps(P, N, L=5, S=4, seed=0):
    return torch.softmax(torch.randn(P, N, L, S, generator=torch.Generator().manual_seed(seed)), dim=2)


def test_stack_timestamp_layout():
    prs = [(2, 6), (3, 10), (3, 11)]
    m = _maps(3, 1)
    w = align.stack(m, prs, 1, 16, torch.bfloat16)
    assert w.shape == (4, 16, 5, 4) and w.dtype == torch.bfloat16   # squeezed: [layers, H, L, S]
    for i, (l, h) in enumerate(prs):
        assert torch.equal(w[l, h], m[i, 0].to(torch.bfloat16))     # the reference's .to(query.dtype)
    mask = torch.ones(4, 16, dtype=torch.bool)
    for l, h in prs:
        mask[l, h] = False
    assert not w[mask].any()
    w2 = align.stack(_maps(3, 2), prs, 2, 16, torch.float32)
    assert w2.shape == (4, 2, 16, 5, 4) and w2.dtype == torch.float32   # bsz > 1: [layers, item, H, L, S], as the reference


def test_stack_score_split():
    prs = [(0, 1), (1, 0)]
    m = _maps(2, 4)
    lm, dit = align.stack(m, prs, 2, 2, torch.float32)
    assert lm.shape == dit.shape == (2, 2, 2, 5, 4)
    assert torch.equal(lm[0, :, 1], m[0, :2]) and torch.equal(dit[1, :, 0], m[1, 2:])
    lm1, dit1 = align.stack(m[:, :2], prs, 1, 2, torch.float32)
    assert lm1.shape == (2, 2, 5, 4) and torch.equal(dit1[1, 0], m[1, 1])
    with pytest.raises(ValueError):
        align.stack(m, prs, 3, 2, torch.float32)


# ------------------------------------------------------------------------------------------------ the mixin on a stub host
class _Tok:
    def encode(self, text, add_special_tokens=False):
        assert not add_special_tokens
        return list(range(len(text.split())))   # "# Languages\nen\n\n# Lyric\n" -> 5 tokens


class _FakeDit:
    """Stands for NativeDit: canned maps, records its calls."""

    def __init__(self, fail=False):
        self.cfg = ace355.DitConfig(**TINY)
        self.device = torch.device("cpu")
        self.fail, self.calls, self.slots = fail, [], {}

    def set_condition(self, slot, enc, L=None):
        self.slots[slot] = enc.shape

    def cross_attention_maps(self, x, ctx, t, t_r, slots, prs):
        if self.fail:
            raise RuntimeError("native failure")
        self.calls.append((x.clone(), ctx.clone(), list(t), list(slots), list(prs)))
        N, T = x.shape[:2]
        return _maps(len(prs), N, 12, (T + 1) // 2)


@pytest.fixture
def fake_scoring(monkeypatch):
    seen = {}

    class MusicStampsAligner:
        def __init__(self, tok):
            seen["tok"] = tok

        def stamps_align_info(self, attention_matrix, lyrics_tokens, total_duration_seconds, custom_config, return_matrices,
                              violence_level, medfilt_width):
            seen["ts"] = (attention_matrix, lyrics_tokens, custom_config)
            return {"calc_matrix": np.ones((2, 2))}

        def get_timestamps_and_lrc(self, calc_matrix, lyrics_tokens, total_duration_seconds):
            return {"lrc_text": "[00:00.00]la", "sentence_timestamps": [1], "token_timestamps": [2]}

    class MusicLyricScorer:
        def __init__(self, tok):
            pass

        def lyrics_alignment_info(self, attention_matrix, token_ids, custom_config, return_matrices, medfilt_width):
            seen.setdefault("score", []).append(attention_matrix)
            return {"energy_matrix": 1, "type_mask": 2, "path_coords": 3}

        def calculate_score(self, energy_matrix, type_mask, path_coords):
            return {"lyrics_score": 0.25 * len(seen["score"])}

    mods = {"acestep": types.ModuleType("acestep"), "acestep.core": types.ModuleType("acestep.core"),
            "acestep.core.scoring": types.ModuleType("acestep.core.scoring"),
            "acestep.core.scoring.dit_alignment": types.ModuleType("acestep.core.scoring.dit_alignment"),
            "acestep.core.scoring.dit_score": types.ModuleType("acestep.core.scoring.dit_score")}
    mods["acestep.core.scoring.dit_alignment"].MusicStampsAligner = MusicStampsAligner
    mods["acestep.core.scoring.dit_score"].MusicLyricScorer = MusicLyricScorer
    for k, v in mods.items():
        monkeypatch.setitem(sys.modules, k, v)
    return seen


class _Parent:
    """The host's PyTorch methods (LyricTimestampMixin / LyricScoreMixin further up the MRO)."""

    def get_lyric_timestamp(self, **kw):
        self.parent_call = ("timestamp", kw)
        return {"from": "parent"}

    def get_lyric_score(self, **kw):
        self.parent_call = ("score", kw)
        return {"from": "parent"}


class _Host(NativeDitMixin, _Parent):
    def __init__(self, dit):
        self.native_dit, self.use_native_dit = dit, True
        self.device, self.dtype = "cpu", torch.bfloat16
        self.text_tokenizer = _Tok()


class _Orphan(NativeDitMixin):
    def __init__(self, dit):
        self.native_dit, self.use_native_dit = dit, True
        self.device, self.dtype = "cpu", torch.bfloat16
        self.text_tokenizer = _Tok()


def _args(B=1, T=9, L=12):
    g = torch.Generator().manual_seed(7)
    return dict(pred_latent=torch.randn(B, T, 64, generator=g), encoder_hidden_states=torch.randn(B, L, 256, generator=g),
                encoder_attention_mask=torch.ones(B, L), context_latents=torch.randn(B, T, 128, generator=g),
                lyric_token_ids=torch.tensor([[0, 1, 2, 3, 4, 10, 11, 12, 151643, 0]]))


CFG = {0: [1], 1: [0, 1]}


def test_timestamp_payload(fake_scoring):
    host = _Host(_FakeDit())
    res = host.get_lyric_timestamp(**_args(), total_duration_seconds=30.0, inference_steps=8, seed=42, custom_layers_config=CFG)
    assert res == {"lrc_text": "[00:00.00]la", "sentence_timestamps": [1], "token_timestamps": [2], "success": True, "error": None}
    m, ids, cfg = fake_scoring["ts"]
    assert m.dtype == torch.bfloat16 and m.shape == (2, 2, 3, 5)   # [layers, H, lyric rows 5:8, S]
    assert ids == [10, 11, 12] and cfg == CFG
    x, ctx, t, slots, prs = host.native_dit.calls[0]
    assert slots == [0] and prs == [(0, 1), (1, 0), (1, 1)] and t == [float(torch.tensor(0.125, dtype=torch.bfloat16))]
    a = _args()
    noise = align.noise_like(a["pred_latent"].to(torch.bfloat16), 42)
    assert torch.equal(x, (0.125 * noise + 0.875 * a["pred_latent"].to(torch.bfloat16)).float())


def test_score_payload(fake_scoring):
    host = _Host(_FakeDit())
    res = host.get_lyric_score(**_args(), inference_steps=8, seed=1, custom_layers_config=CFG)
    assert res == {"lm_score": 0.25, "dit_score": 0.5, "success": True, "error": None}
    lm, dit = fake_scoring["score"]
    assert lm.shape == dit.shape == (2, 2, 3, 5) and lm.dtype == torch.bfloat16
    x, ctx, t, slots, prs = host.native_dit.calls[0]
    assert slots == [0, 0] and t[0] == 1.0 and x.shape[0] == 2 and ctx.shape[0] == 2


def test_host_default_config(fake_scoring):
    host = _Host(_FakeDit())
    host.custom_layers_config = {1: [1]}
    host.get_lyric_timestamp(**_args(), total_duration_seconds=30.0)
    assert host.native_dit.calls[0][4] == [(1, 1)] and fake_scoring["ts"][2] == {1: [1]}


@pytest.mark.parametrize("steps", [0, -2, 1.5])
def test_bad_steps_payloads(steps):
    host = _Host(_FakeDit())
    r = host.get_lyric_timestamp(**_args(), total_duration_seconds=30.0, inference_steps=steps, custom_layers_config=CFG)
    assert r == {"lrc_text": "", "sentence_timestamps": [], "token_timestamps": [], "success": False,
                 "error": f"inference_steps must be a positive non-zero integer, got {steps!r}"}
    r = host.get_lyric_score(**_args(), inference_steps=steps, custom_layers_config=CFG)
    assert r == {"lm_score": 0.0, "dit_score": 0.0, "success": False,
                 "error": f"Error generating score: inference_steps must be a positive non-zero integer, got {steps!r}"}
    assert not host.native_dit.calls


def test_raising_native_part_falls_back_to_super():
    host = _Host(_FakeDit(fail=True))
    a = _args()
    assert host.get_lyric_timestamp(**a, total_duration_seconds=12.5, vocal_language="fr", inference_steps=4, seed=3,
                                    custom_layers_config=CFG) == {"from": "parent"}
    kind, kw = host.parent_call
    assert kind == "timestamp" and kw["total_duration_seconds"] == 12.5 and kw["vocal_language"] == "fr" and kw["inference_steps"] == 4
    assert kw["seed"] == 3 and kw["custom_layers_config"] is CFG and kw["pred_latent"] is a["pred_latent"]
    assert host.get_lyric_score(**a, inference_steps=4, seed=3) == {"from": "parent"}
    assert host.parent_call[0] == "score" and host.parent_call[1]["custom_layers_config"] is None


def test_inactive_native_dit_uses_super():
    host = _Host(None)
    host.use_native_dit = False
    assert host.get_lyric_timestamp(**_args(), total_duration_seconds=1.0) == {"from": "parent"}
    assert host.get_lyric_score(**_args()) == {"from": "parent"}


def test_no_super_gives_the_error_payload(monkeypatch):
    host = _Orphan(_FakeDit(fail=True))
    r = host.get_lyric_timestamp(**_args(), total_duration_seconds=1.0, custom_layers_config=CFG)
    assert r["success"] is False and r["lrc_text"] == "" and "native failure" in r["error"]
    r = host.get_lyric_score(**_args(), custom_layers_config=CFG)
    assert r["success"] is False and r["lm_score"] == 0.0 and "native failure" in r["error"]
    host.use_native_dit = False
    assert host.get_lyric_score(**_args())["success"] is False


def test_missing_scoring_package_gives_the_error_payload(monkeypatch):
    monkeypatch.setitem(sys.modules, "acestep", None)   # import acestep.* raises ImportError
    host = _Orphan(_FakeDit())
    r = host.get_lyric_timestamp(**_args(), total_duration_seconds=1.0, custom_layers_config=CFG)
    assert r["success"] is False and r["error"].startswith("Error generating timestamps:")
    host.text_tokenizer = None
    r = host.get_lyric_score(**_args(), custom_layers_config=CFG)
    assert r["success"] is False and "text_tokenizer" in r["error"]


def test_native_handler_defaults():
    from ace355.backend import NativeHandler
    h = NativeHandler()
    assert h.custom_layers_config == align.DEFAULT_LAYERS_HEADS
    r = h.get_lyric_timestamp(**_args(), total_duration_seconds=1.0)   # not initialised: no backend, the payload, no exception
    assert r["success"] is False


# ------------------------------------------------------------------------------------------------ tiny G18 case vs the oracle
def test_g18_tiny_oracle(golden_dir):
    from ace355 import weightgen
    from oracle import dit as o_dit
    G = np.load(os.path.join(golden_dir, "g18_alignment.npz"))
    assert float(G["bound"]) == G18_ORACLE_BOUND
    cfg = o_dit.DitConfig(**TINY)
    w = weightgen.make_dit_weights(o_dit.dit_weight_shapes(cfg), cfg.hidden_size, seed=int(G["tiny_seed"]), mode="test")
    assert weightgen.checksum(w) == pytest.approx(float(G["tiny_wsum"]), rel=1e-9)
    pred, noise, ctx, enc = g18_inputs(int(G["tiny_T"]), int(G["tiny_L"]), cfg.hidden_size, int(G["tiny_input_seed"]))
    assert np.allclose(checksum(pred, noise, ctx, enc), G["tiny_input_sums"], rtol=1e-9)
    x, t = g18_score_rows(pred, noise)
    assert torch.equal(t, torch.from_numpy(G["tiny_t"]))
    prs = [tuple(int(v) for v in p) for p in G["tiny_pairs"]]
    with capture_cross(o_dit) as cap, torch.no_grad():
        o_dit.dit_forward(cfg, w, x, t, t, torch.cat([enc, enc]), torch.cat([ctx, ctx]))
    d = float((handler_layout(cap, prs) - torch.from_numpy(G["tiny_maps"])).abs().max())
    assert d < G18_ORACLE_BOUND, d
