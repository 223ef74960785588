"""GPU: the native LM token selection (``ace355_lm_pick`` through ace355.lmsample and the ``NativeLmMixin`` seam) against fixture G22
and the fp64 restatement tests/_lm_sample_oracle.py.

Keep masks, kept counts and tokens are compared EXACTLY.  That is fair because every input's top-p walk keeps its prefix masses at least
1e-4 (G22: 1e-3) away from p - asserted on the inputs here - while the native path and the oracle both work in fp64 and differ by
rounding of sums only (about 3e-7 at the very most, were one of them fp32).  Rows of plain ``randn * 3`` at the real vocabulary cannot
meet that margin (their prefix masses near the cut are closer together than it), so large rows carry a few planted peaks among which the
cut falls.  Everything is random logits; nothing about a trained LM's token stream is pinned.
"""
import numpy as np
import pytest
import torch

import _lm_sample_oracle as O

pytestmark = pytest.mark.gpu

MARGIN = 1e-4
SETTINGS = [(None, 0.9), (50, None), (200, 0.95), (None, None)]
REAL_V = 217205


def draw_rows(V, B, seed, settings=SETTINGS, peaks=8):
    """[B, V] float32: ``randn * 3`` with ``peaks`` planted large entries per row (V > 64), each row re-drawn until its top-p walk
    keeps the margin under every setting."""
    rows, s = [], seed * 1000
    while len(rows) < B:
        s += 1
        g = np.random.default_rng(s)
        x = (g.standard_normal(V) * 3).astype(np.float32)
        if V > 64:
            x[g.choice(V, peaks, replace=False)] = (20.0 + 4.0 * g.random(peaks)).astype(np.float32)
        if all(O.top_p_margin(x, k, p)[0] >= MARGIN for k, p in settings):
            rows.append(x)
    return np.stack(rows)


def native_pick(x, k, p, T=0.0, u=None):
    from ace355 import lmsample
    tokens, kept, keep = lmsample.pick(x, k, p, T, u, want_kept=True, want_mask=True)
    return tokens.cpu().numpy(), kept.cpu().numpy(), keep.cpu().numpy().astype(bool)


def midpoint_u(x, keep, T, which):
    """fp32 u at the middle of the CDF interval of the ``which``-th kept id that owns a sizable interval (> 1e-3 of the mass)."""
    ids, w, c = O.cdf(x, keep, T)
    wide = np.nonzero(w / c[-1] > 1e-3)[0]
    i = wide[which % wide.shape[0]]
    return np.float32((c[i] - 0.5 * w[i]) / c[-1])


def check_against_oracle(xnp, x, k, p, T=0.85):
    B = xnp.shape[0]
    for r in range(B):
        dist, _ = O.top_p_margin(xnp[r], k, p)
        assert dist >= MARGIN, (r, k, p, dist)
    masks = [O.keep_mask(xnp[r], k, p) for r in range(B)]
    tok, kept, keep = native_pick(x, k, p)
    for r in range(B):
        assert np.array_equal(keep[r], masks[r]), (r, k, p, int(keep[r].sum()), int(masks[r].sum()))
        assert kept[r] == masks[r].sum() and tok[r] == O.greedy_token(xnp[r], masks[r]), (r, k, p)
    u = np.array([midpoint_u(xnp[r], masks[r], T, r) for r in range(B)], dtype=np.float32)
    tok, kept, keep2 = native_pick(x, k, p, T, torch.from_numpy(u))
    assert np.array_equal(keep2, keep)
    for r in range(B):
        assert tok[r] == O.token_for_u(xnp[r], masks[r], T, u[r]) and kept[r] == masks[r].sum(), (r, k, p, float(u[r]))


# ------------------------------------------------------------------ G22
def test_every_g22_case(gpu_device):
    for c, (xnp, sets) in enumerate(O.load_g22()):
        x = torch.from_numpy(xnp).to(gpu_device)
        for k, p, fin, greedy in sets:
            tok, kept, keep = native_pick(x, k, p)
            assert np.array_equal(keep, fin), (c, k, p, keep.sum(1).tolist(), fin.sum(1).tolist())
            assert np.array_equal(kept, fin.sum(1)) and np.array_equal(tok, greedy), (c, k, p)
        assert torch.equal(x.cpu(), torch.from_numpy(xnp))


# ------------------------------------------------------------------ sizes
def _edge_sizes():
    from ace355 import native
    chunk = native.lm_pick_plan(1)["chunk"]
    return [n * chunk + d for n in (1, 2) for d in (-1, 0, 1)]   # around the edges of the two smallest chunk counts


@pytest.mark.parametrize("B", [1, 3, 16])
def test_sizes_around_chunk_edges(gpu_device, B):
    from ace355 import native
    for V in _edge_sizes():
        chunk = native.lm_pick_plan(V)["chunk"]
        assert native.lm_pick_plan(V)["chunks"] == -(-V // chunk)
        xnp = draw_rows(V, B, seed=V + B)
        x = torch.from_numpy(xnp).to(gpu_device)
        for k, p in SETTINGS:
            check_against_oracle(xnp, x, k, p)


def test_real_vocabulary(gpu_device):
    xnp = draw_rows(REAL_V, 2, seed=7)
    xnp[1, :64000] = -np.inf    # the second row in the codes phase: only the upper ids (and whatever peaks fell there) are finite
    xnp[1, 100] = 21.5          # ... plus one low "EOS" id
    for k, p in SETTINGS:
        assert O.top_p_margin(xnp[1], k, p)[0] >= MARGIN
    x = torch.from_numpy(xnp).to(gpu_device)
    for k, p in SETTINGS:
        check_against_oracle(xnp, x, k, p)


def test_strided_rows(gpu_device):
    V, B = 1003, 3
    wide = torch.full((B, V + 37), float("nan"), device=gpu_device)   # what lies beside the slice must never be read
    xnp = draw_rows(V, B, seed=11)
    x = wide[:, 20:20 + V]
    x.copy_(torch.from_numpy(xnp))
    assert x.stride(0) == V + 37 and not x.is_contiguous()
    for k, p in SETTINGS:
        check_against_oracle(xnp, x, k, p)


# ------------------------------------------------------------------ sampling
@pytest.mark.parametrize("V", [65, 1003])
@pytest.mark.parametrize("T", [0.05, 0.85, 1.0, 2.0])
def test_inverse_cdf_matches_oracle_inside_every_interval(gpu_device, V, T):
    """Every kept token's fp32 CDF midpoint, and the points 1e-6 of the mass inside each edge of every interval wider than 1e-5."""
    xnp = (np.random.default_rng(100 + V).standard_normal(V) * 3).astype(np.float32)
    for k, p in ((None, None), (None, 0.9)):
        assert O.top_p_margin(xnp, k, p)[0] >= MARGIN
        keep = O.keep_mask(xnp, k, p)
        ids, w, c = O.cdf(xnp, keep, T)
        W = c[-1]
        wide = w / W > 1e-5
        assert w[~wide].sum() / W <= 0.01    # the skipped intervals carry at most 1 % of the mass
        lo, hi = (c - w)[wide] / W, c[wide] / W
        u = np.concatenate([(lo + hi) / 2, lo + 1e-6, hi - 1e-6]).astype(np.float32)
        u = u[u < 1.0]
        want = ids[np.searchsorted(c, u.astype(np.float64) * W, side="right")]
        assert np.array_equal(want[:int(wide.sum())], ids[wide])
        x = torch.from_numpy(xnp).to(gpu_device)[None].expand(16, V)
        got = []
        for i in range(0, u.shape[0], 16):
            ui = np.resize(u[i:i + 16], 16)
            tok, _kept, _keep = native_pick(x, k, p, T, torch.from_numpy(ui))
            got.append(tok[:min(16, u.shape[0] - i)])
        got = np.concatenate(got)
        assert np.array_equal(got, want), (k, p, np.nonzero(got != want)[0][:5].tolist())


def test_u_at_both_ends(gpu_device):
    xnp = draw_rows(1003, 1, seed=3)[0]
    x = torch.from_numpy(xnp).to(gpu_device)[None]
    keep = O.keep_mask(xnp, None, 0.9)
    ids, w, c = O.cdf(xnp, keep, 1.0)
    assert ids.shape[0] >= 3 and (w / c[-1] > 1e-3).all()   # every kept id owns a sizable interval
    below_one = np.nextafter(np.float32(1), np.float32(0))
    for u, want in ((np.float32(0), ids[0]), (below_one, ids[-1])):
        assert O.token_for_u(xnp, keep, 1.0, u) == want
        tok, _kept, _keep = native_pick(x, None, 0.9, 1.0, torch.tensor([u]))
        assert tok[0] == want


# ------------------------------------------------------------------ ties and zeros
def test_cut_inside_a_tie_group_takes_ascending_ids(gpu_device):
    one = np.full(1003, 1.25, dtype=np.float32)                 # one chunk
    spread = np.full(20000, -np.inf, dtype=np.float32)          # 1000 equal entries over three chunks
    spread[7::20] = -3.5
    for xnp, p in ((one, 0.9), (spread, 0.9005), (spread, 0.4105)):
        dist, _ = O.top_p_margin(xnp, None, p)
        assert dist >= MARGIN
        keep = O.keep_mask(xnp, None, p)
        fin = np.nonzero(np.isfinite(xnp))[0]
        n = int(keep.sum())
        assert 1 < n < fin.shape[0] and np.array_equal(np.nonzero(keep)[0], fin[:n])   # the oracle's rule: the first n ids of the group
        tok, kept, got = native_pick(torch.from_numpy(xnp).to(gpu_device)[None], None, p)
        assert np.array_equal(got[0], keep) and kept[0] == n and tok[0] == fin[0]


def test_signed_zeros_are_one_value(gpu_device):
    xnp = np.full(65, -2.0, dtype=np.float32)
    xnp[[3, 9, 20, 40]] = [3.0, 2.0, 0.0, -0.0]
    x = torch.from_numpy(xnp).to(gpu_device)[None]
    for k, n in ((3, 4), (4, 4), (2, 2)):    # the zeros straddle the k-th place: both kept, or both dropped
        tok, kept, keep = native_pick(x, k, None)
        assert np.array_equal(keep[0], O.keep_mask(xnp, k, None)) and kept[0] == n and keep[0][20] == keep[0][40]
    xnp[[3, 9]] = -5.0                        # the zeros are the maximum: the lower id wins whatever its sign
    x = torch.from_numpy(xnp).to(gpu_device)[None]
    assert native_pick(x, None, None)[0][0] == 20
    xnp[[20, 40]] = [-0.0, 0.0]
    assert native_pick(torch.from_numpy(xnp).to(gpu_device)[None], None, None)[0][0] == 20


# ------------------------------------------------------------------ bad rows
def test_bad_rows_are_data(gpu_device):
    from ace355 import lmsample
    V = 8193
    good = draw_rows(V, 1, seed=21)[0]
    nan_row, inf_row = good.copy(), good.copy()
    nan_row[V - 1] = np.nan
    inf_row[0] = np.inf
    xnp = np.stack([nan_row, good, inf_row, np.full(V, -np.inf, dtype=np.float32)])
    x = torch.from_numpy(xnp).to(gpu_device)
    u = torch.full((4,), 0.37)
    for k, p in SETTINGS:
        for T in (0.0, 0.85):
            tok, kept, keep = native_pick(x, k, p, T, u)
            alone = native_pick(x[1:2], k, p, T, u[1:2])
            assert tok.tolist() == [-1, int(alone[0][0]), -1, -1] and kept.tolist() == [0, int(alone[1][0]), 0, 0]
            assert not keep[[0, 2, 3]].any() and np.array_equal(keep[1], alone[2][0])
            assert np.array_equal(keep[1], O.keep_mask(good, k, p)) and tok[1] == O.token_for_u(good, keep[1], T, 0.37)
    with pytest.raises(RuntimeError, match="rows \\[0, 2, 3\\]"):
        lmsample.select_tokens(x, top_p=0.9, temperature=0.85)
    assert lmsample.select_tokens(x, top_p=0.9, temperature=0.85, check=False).tolist()[0] == -1
    assert lmsample.select_tokens(x[1:2], top_p=0.9, temperature=0.0).tolist() == [O.greedy_token(good, np.isfinite(good))]


# ------------------------------------------------------------------ independence and reproducibility
def test_rows_do_not_see_each_other(gpu_device):
    V = 16385
    xnp = draw_rows(V, 16, seed=31)
    x = torch.from_numpy(xnp).to(gpu_device)
    before = x.clone()
    u = torch.rand(16, generator=torch.Generator().manual_seed(1))
    for k, p in SETTINGS:
        full = native_pick(x, k, p, 0.85, u)
        again = native_pick(x, k, p, 0.85, u)
        assert all(np.array_equal(a, b) for a, b in zip(full, again))
        for B in (1, 3):
            for r0 in (0, 5, 16 - B):
                part = native_pick(x[r0:r0 + B], k, p, 0.85, u[r0:r0 + B])
                assert all(np.array_equal(a[r0:r0 + B], b) for a, b in zip(full, part)), (k, p, B, r0)
    assert torch.equal(x, before)


def test_more_rows_than_one_call_and_other_dtypes(gpu_device):
    from ace355 import lmsample
    xnp = draw_rows(1003, 37, seed=41)
    x = torch.from_numpy(xnp).to(gpu_device)
    tok, mask = lmsample.select_tokens(x, top_k=50, top_p=0.95, temperature=0.0, return_mask=True)
    assert mask.dtype == torch.bool and tok.dtype == torch.int64
    for r in range(37):
        keep = O.keep_mask(xnp[r], 50, 0.95)
        assert np.array_equal(mask[r].cpu().numpy(), keep) and int(tok[r]) == O.greedy_token(xnp[r], keep)
    xb = x.to(torch.bfloat16)     # upcast as the reference upcasts: the selection is that of the rounded values
    tok = lmsample.select_tokens(xb, top_k=50, temperature=0.0)
    assert tok.tolist() == [int(np.argmax(row)) for row in xb.float().cpu().numpy()]   # (the first position of the maximum)


# ------------------------------------------------------------------ filter_logits_
def test_filter_logits_in_place(gpu_device):
    from ace355 import lmsample
    xnp = draw_rows(2051, 3, seed=51)
    for k, p in SETTINGS:
        x = torch.from_numpy(xnp).to(gpu_device)
        out = lmsample.filter_logits_(x, k, p)
        assert out is x
        keep = np.stack([O.keep_mask(xnp[r], k, p) for r in range(3)])
        want = torch.from_numpy(xnp).masked_fill(torch.from_numpy(~keep), float("-inf"))
        assert torch.equal(x.cpu(), want)


# ------------------------------------------------------------------ the seam
class _Base:
    """Restates the three reference methods (llm_inference.py:367-399) and counts its calls."""

    def __init__(self):
        self.calls = []

    def _apply_top_k_filter(self, logits, top_k):
        self.calls.append("k")
        if top_k is not None and top_k > 0:
            logits[logits < torch.topk(logits, top_k)[0][..., -1, None]] = float("-inf")
        return logits

    def _apply_top_p_filter(self, logits, top_p):
        self.calls.append("p")
        if top_p is not None and 0.0 < top_p < 1.0:
            s, idx = torch.sort(logits, descending=True)
            rem = torch.cumsum(torch.softmax(s.float(), dim=-1), dim=-1) > top_p
            rem[..., 1:] = rem[..., :-1].clone()
            rem[..., 0] = 0
            logits[rem.scatter(1, idx, rem)] = float("-inf")
        return logits

    def _sample_tokens(self, logits, temperature):
        self.calls.append("s")
        if temperature > 0:
            return torch.multinomial(torch.softmax(logits.float() / temperature, dim=-1), num_samples=1).squeeze(1)
        return torch.argmax(logits, dim=-1)


def _handler(flag):
    from ace355.backend import NativeLmMixin

    class Handler(NativeLmMixin, _Base):
        pass

    h = Handler()
    h.use_native_lm_sampler = flag
    return h


def _step(h, x, k, p, T):
    """As the reference's loops drive the seam: k, then p, then the draw, on one tensor."""
    t = h._apply_top_k_filter(x, k)
    t = h._apply_top_p_filter(t, p)
    return h._sample_tokens(t, T)


def test_seam_runs_the_fused_call(gpu_device):
    from ace355 import lmsample
    xnp = draw_rows(2051, 8, seed=61)
    x = torch.from_numpy(xnp).to(gpu_device)
    h = _handler(True)
    for k, p, T in ((50, 0.95, 0.85), (0, 0.9, 0.85), (None, None, 2.0), (50, 0.95, 0.0)):
        torch.manual_seed(9)
        got = _step(h, x, k, p, T)
        torch.manual_seed(9)
        u = torch.rand(8, device=gpu_device)
        assert torch.equal(got, lmsample.select_tokens(x, k, p, T, u=u))
        if T > 0:
            masks = [O.keep_mask(xnp[r], k or None, p) for r in range(8)]
            assert got.tolist() == [O.token_for_u(xnp[r], masks[r], T, float(u[r])) for r in range(8)]
    assert h.calls == [] and torch.equal(x.cpu(), torch.from_numpy(xnp)) and h._lm_sampler_record is None


def test_seam_applies_no_stale_filter(gpu_device):
    from ace355 import lmsample
    a = torch.from_numpy(draw_rows(2051, 8, seed=71)).to(gpu_device)
    b = torch.from_numpy(draw_rows(2051, 8, seed=72, settings=[(None, None)], peaks=0)).to(gpu_device)
    h = _handler(True)
    h._apply_top_k_filter(a, 1)
    h._apply_top_p_filter(a, 0.5)
    torch.manual_seed(4)
    got = h._sample_tokens(b, 2.0)          # another tensor: the caller filtered it elsewhere, or not at all
    torch.manual_seed(4)
    assert torch.equal(got, lmsample.select_tokens(b, None, None, 2.0))
    assert not torch.equal(got, b.argmax(-1))   # (top-k 1 would have forced the maximum on every row)
    assert h._lm_sampler_record is None
    # a record for a tensor that was never sampled is dropped by the next step's filters, not merged into them
    h._apply_top_k_filter(a, 1)
    torch.manual_seed(4)
    got = _step(h, b, None, None, 2.0)
    torch.manual_seed(4)
    assert torch.equal(got, lmsample.select_tokens(b, None, None, 2.0)) and h.calls == []


def test_seam_off_and_fallback_use_the_base_path(gpu_device, monkeypatch):
    from ace355 import lmsample
    xnp = draw_rows(1003, 3, seed=81)
    off, ref = _handler(False), _Base()
    x, y = torch.from_numpy(xnp).to(gpu_device), torch.from_numpy(xnp).to(gpu_device)
    torch.manual_seed(2)
    got = _step(off, x, 50, 0.95, 0.85)
    torch.manual_seed(2)
    assert torch.equal(got, _step(ref, y, 50, 0.95, 0.85)) and off.calls == ["k", "p", "s"] and torch.equal(x, y)

    def boom(*a, **k):
        raise RuntimeError("native call failed")
    monkeypatch.setattr(lmsample, "select_tokens", boom)
    on = _handler(True)
    x = torch.from_numpy(xnp).to(gpu_device)
    for _ in range(5):
        x.copy_(torch.from_numpy(xnp))
        torch.manual_seed(2)
        assert torch.equal(_step(on, x, 50, 0.95, 0.85), got)      # the deferred filters ran first, then the base draw
        assert torch.equal(x, y)
    assert on.calls == ["k", "p", "s"] * 5 and on._lm_sampler_failures == 5
