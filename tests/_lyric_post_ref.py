"""CPU restatement of the lyric alignment stage after the cross-attention maps, written from the behaviour of the reference's
``MusicStampsAligner`` / ``MusicLyricScorer`` / ``dtw_cpu`` (acestep/core/scoring) and pinned to their recorded results by
tests/golden/g20_lyric_post.npz (tests/test_align_post_cpu.py).

Two variants of everything up to the matrix the DTW reads: ``ref32`` (``dtype=torch.float32``) computes in the reference's own dtypes,
``ref64`` (``dtype=torch.float64``) in fp64 throughout.  The DTW always keeps the reference's fp32 cost table.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------------------------ inputs
def ridge_maps(H: int, L: int, S: int, seed: int) -> torch.Tensor:
    """fp32 [H, L, S]: softmax over the L keys of randn + a monotone ridge (frame s attends to token s L / S), as a map is laid out."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(H, S, L, generator=g).double()
    s = torch.arange(S, dtype=torch.float64)[:, None]
    l = torch.arange(L, dtype=torch.float64)[None]
    logits = logits + 6.0 * torch.exp(-0.5 * ((l - s * L / S) / 1.5) ** 2)
    return torch.softmax(logits, -1).transpose(-1, -2).contiguous().float()


class ToyTokenizer:
    """Byte-level toy vocabulary: words, a newline, bracket tags and one three-byte character split over two tokens."""
    VOCAB = [b"la", b" ", b"\n", b"[", b"verse", b"]", b"\xe4\xb8", b"\xad", b"oh", b"na", b"!\n"]
    PHRASE = [3, 4, 5, 2, 0, 1, 9, 1, 6, 7, 2, 8, 1, 0, 10, 9, 1, 9, 1, 0, 2]

    def decode(self, ids, skip_special_tokens=False):
        return b"".join(self.VOCAB[i] for i in ids).decode("utf-8", errors="replace")

    def encode(self, text, add_special_tokens=False):
        return list(range(len(text.split())))

    @classmethod
    def ids(cls, n: int):
        return [cls.PHRASE[i % len(cls.PHRASE)] for i in range(n)]


# ------------------------------------------------------------------------------------------------------------------ matrices
def median_filter(x: torch.Tensor, w: int) -> torch.Tensor:
    """Width-w median along the last axis with reflect padding; the identity when the axis is no longer than w // 2."""
    pad = w // 2
    if x.shape[-1] <= pad:
        return x
    lead = x.shape[:-1]
    y = F.pad(x.reshape(1, -1, x.shape[-1]), (pad, pad), mode="reflect")
    return y.unfold(-1, w, 1).sort()[0][..., pad].reshape(*lead, -1)


def timestamp_matrix(maps: torch.Tensor, violence_level: float = 2.0, medfilt_width: int = 1, dtype=torch.float32):
    """maps [H, R, S] -> (calc, energy) numpy [R, S] in ``dtype``: the bidirectional consensus filter."""
    x = maps.to(dtype)
    p = torch.softmax(x, -1) * torch.softmax(x, -2)
    p = torch.relu(p - violence_level * torch.quantile(p, 0.5, dim=-1, keepdim=True))
    p = torch.relu(p - violence_level * torch.quantile(p, 0.5, dim=-2, keepdim=True))
    p = p ** 2
    energy = p.mean(0)
    std, mean = torch.std_mean(p, unbiased=False)
    z = median_filter((p - mean) / (std + 1e-9), medfilt_width)
    return z.mean(0).numpy(), energy.numpy()


def score_matrix(maps: torch.Tensor, medfilt_width: int = 1, dtype=torch.float32):
    """maps [H, R, S] -> (calc, energy): head mean, median filter, min-max normalisation; calc = energy ** 2."""
    e = median_filter(maps.to(dtype).mean(0), medfilt_width).numpy()
    lo, hi = e.min(), e.max()
    e = (e - lo) / (hi - lo) if hi - lo > 1e-9 else np.zeros_like(e)
    return e ** 2, e


# ------------------------------------------------------------------------------------------------------------------ DTW
def dtw(x: np.ndarray):
    """The path of least cost through x [N, M] from (0, 0) to (N - 1, M - 1): fp32 cost table, steps diagonal / up / left chosen in
    that order with strict comparisons (diagonal only if below both others, else up only if below both others, else left).
    Returns (row indices, column indices) int32.  Cells are visited along anti-diagonals; each cell's arithmetic is the plain
    column-by-column loop's."""
    N, M = x.shape
    x = np.asarray(x)
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    trace = np.full((N + 1, M + 1), -1, dtype=np.int8)
    cost[0, 0] = 0
    for d in range(2, N + M + 1):
        i = np.arange(max(1, d - M), min(N, d - 1) + 1)
        j = d - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        diag = (c0 < c1) & (c0 < c2)
        up = ~diag & (c1 < c0) & (c1 < c2)
        c = np.where(diag, c0, np.where(up, c1, c2))
        cost[i, j] = (x[i - 1, j - 1] + c).astype(np.float32)
        trace[i, j] = np.where(diag, 0, np.where(up, 1, 2))
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j, rows, cols = N, M, [], []
    while i > 0 or j > 0:
        rows.append(i - 1)
        cols.append(j - 1)
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return np.array(rows[::-1], dtype=np.int32), np.array(cols[::-1], dtype=np.int32)


def token_frames(rows: np.ndarray, cols: np.ndarray, R: int) -> np.ndarray:
    """int32 [R, 2]: the first and last column on the path of each row, -1 for a row the path skips."""
    out = np.full((R, 2), -1, dtype=np.int32)
    for r in range(R):
        c = cols[rows == r]
        if len(c):
            out[r] = (c[0], c[-1])
    return out


def path_cost(x: np.ndarray, rows, cols) -> float:
    return float(np.asarray(x, dtype=np.float64)[np.asarray(rows), np.asarray(cols)].sum())


# ------------------------------------------------------------------------------------------------------------------ score
def score_metrics(energy, path_coords, type_mask, time_weight=0.01, overlap_frames=9.0, instrumental_weight=1.0):
    """(coverage, monotonicity, path confidence) in fp64 from energy [R, S] (read as fp32), path [len, 2], mask [R]."""
    e = torch.as_tensor(np.asarray(energy, dtype=np.float32)).double()
    path = torch.as_tensor(np.asarray(path_coords)).long().reshape(-1, 2)
    mask = torch.as_tensor(np.asarray(type_mask)).long()
    lyric = mask == 1
    n_lyric = int(lyric.sum())
    coverage = float((lyric & (e.max(1).values > 0.1)).sum()) / n_lyric if n_lyric else 1.0
    w = torch.where(e > time_weight, e, torch.zeros_like(e))
    sw = w.sum(1)
    st = (w * torch.arange(e.shape[1], dtype=torch.float64)).sum(1)
    cent = torch.full((e.shape[0],), -1.0, dtype=torch.float64)
    ok = sw > 1e-9
    cent[ok] = st[ok] / sw[ok]
    c = cent[lyric & (cent >= 0)]
    mono = float((c[1:] >= c[:-1] - overlap_frames).double().sum()) / (len(c) - 1) if len(c) > 1 else 1.0
    conf = 0.0
    if len(path):
        pe = e[path[:, 0], path[:, 1]]
        sw_ = torch.ones_like(pe)
        sw_[mask[path[:, 0]] == 0] = instrumental_weight
        if float(sw_.sum()) > 0:
            conf = float((pe * sw_).sum() / sw_.sum())
    return coverage, mono, conf


def final_score(coverage, monotonicity, confidence) -> float:
    return round(float(np.clip((coverage ** 2) * (monotonicity ** 2) * confidence, 0.0, 1.0)), 4)


def type_mask(tokenizer, ids) -> np.ndarray:
    mask = np.ones(len(ids), dtype=np.int32)
    inside = False
    for i, tid in enumerate(ids):
        text = tokenizer.decode([tid])
        if "[" in text:
            inside = True
        if inside:
            mask[i] = 0
        if "]" in text:
            inside, mask[i] = False, 0
    return mask


# ------------------------------------------------------------------------------------------------------------------ a host scoring package
def select(attention_matrix: torch.Tensor, custom_config) -> torch.Tensor:
    """[layers, heads, R, S] -> fp32 [n_pairs, R, S] in the config's order."""
    w = attention_matrix.clone().cpu().float()
    return torch.stack([w[l, h] for l, heads in custom_config.items() for h in heads if l < w.shape[0] and h < w.shape[1]])


def fake_scoring_modules():
    """``acestep.core.scoring`` stand-ins built from ref32 and ``ace355.align_post``'s host-side text pieces: {module name: module}."""
    import types
    from ace355 import align_post

    class MusicStampsAligner:
        def __init__(self, tokenizer):
            self.tokenizer = tokenizer

        def stamps_align_info(self, attention_matrix, lyrics_tokens, total_duration_seconds, custom_config, return_matrices=False,
                              violence_level=2.0, medfilt_width=1):
            calc, _ = timestamp_matrix(select(attention_matrix, custom_config), violence_level, medfilt_width)
            return {"calc_matrix": calc, "lyrics_tokens": lyrics_tokens, "total_duration_seconds": total_duration_seconds}

        def get_timestamps_and_lrc(self, calc_matrix, lyrics_tokens, total_duration_seconds):
            rows, cols = dtw(-calc_matrix.astype(np.float64))
            toks = align_post.token_timestamps(self.tokenizer, lyrics_tokens, token_frames(rows, cols, calc_matrix.shape[0]),
                                               calc_matrix.shape[-1], total_duration_seconds, token_type=align_post.TokenTimestamp)
            sents = align_post.sentence_timestamps(self.tokenizer, toks, sentence_type=align_post.SentenceTimestamp)
            return {"token_timestamps": toks, "sentence_timestamps": sents, "lrc_text": align_post.format_lrc(sents)}

    class MusicLyricScorer:
        def __init__(self, tokenizer):
            self.tokenizer = tokenizer

        def lyrics_alignment_info(self, attention_matrix, token_ids, custom_config, return_matrices=False, medfilt_width=1):
            calc, energy = score_matrix(select(attention_matrix, custom_config), medfilt_width)
            mask = type_mask(self.tokenizer, token_ids)
            if len(mask) != energy.shape[0]:
                mask = np.ones(energy.shape[0], dtype=np.int32)
            rows, cols = dtw(-calc.astype(np.float32))
            return {"path_coords": np.stack([rows, cols], 1), "type_mask": mask, "energy_matrix": energy, "calc_matrix": calc}

        def calculate_score(self, energy_matrix, type_mask, path_coords):
            return {"lyrics_score": final_score(*score_metrics(energy_matrix, path_coords, type_mask))}

    names = ["acestep", "acestep.core", "acestep.core.scoring", "acestep.core.scoring.dit_alignment", "acestep.core.scoring.dit_score"]
    mods = {n: types.ModuleType(n) for n in names}
    mods["acestep.core.scoring.dit_alignment"].MusicStampsAligner = MusicStampsAligner
    mods["acestep.core.scoring.dit_alignment"].TokenTimestamp = align_post.TokenTimestamp
    mods["acestep.core.scoring.dit_alignment"].SentenceTimestamp = align_post.SentenceTimestamp
    mods["acestep.core.scoring.dit_score"].MusicLyricScorer = MusicLyricScorer
    return mods
