"""The lyric alignment stage after the cross-attention maps, on the GPU (include/ace355.h ``ace355_align_*``, csrc/align_post.hip).

The reference hands a ``[layers, 16, L, S]`` stack to ``MusicStampsAligner`` / ``MusicLyricScorer`` (acestep/core/scoring), which copy it
to the host and run two softmaxes, two quantiles, a z-score, a median filter, a DTW and three fp64 reductions there.  Here the same
stages read the fp32 maps ``[n_pairs, N, L, S]`` of ``NativeDit.cross_attention_maps`` where they lie: ``timestamp_matrix`` /
``score_matrix`` -> ``dtw`` -> ``score_metrics``, all device tensors.  What is left for the host is text: the token type mask, the
incremental token decode, seconds from frame indices, sentence grouping and the LRC lines (the second half of this module; no tensors).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Sequence, Tuple

import torch

from . import native


# ------------------------------------------------------------------------------------------------------------------ device functions
def _workspace(n_pairs: int, rows: int, S: int, batch: int, device) -> torch.Tensor:
    nbytes = int(native.lib().ace355_align_workspace_bytes(n_pairs, rows, S, batch))
    if nbytes <= 0:
        raise ValueError(f"align workspace: n_pairs {n_pairs}, rows {rows}, S {S}, batch {batch}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _check_maps(maps: torch.Tensor, item: int, start: int, end: int) -> Tuple[int, int, int, int]:
    if maps.dim() != 4 or maps.dtype != torch.float32 or not maps.is_cuda:
        raise ValueError("maps must be the fp32 device tensor [n_pairs, N, L, S] of cross_attention_maps")
    P, N, L, S = maps.shape
    if not (0 <= item < N and 0 <= start < end <= L):
        raise ValueError(f"item {item} / rows [{start}, {end}) do not fit maps of N = {N}, L = {L}")
    return P, N, L, S


def _round_flag(dtype) -> int:
    if dtype in (torch.float32, None):
        return 0
    if dtype == torch.bfloat16:
        return 1
    raise ValueError(f"dtype {dtype}: the maps are consumed as fp32 or rounded through bf16")


def timestamp_matrix(maps: torch.Tensor, item: int, start: int, end: int, violence_level: float = 2.0, medfilt_width: int = 1,
                     dtype=torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
    """``MusicStampsAligner._apply_bidirectional_consensus`` on rows [start, end) of item ``item``: (calc, energy), fp32 [rows, S] on the
    maps' device.  ``dtype=torch.bfloat16`` rounds the maps through bf16 on load, as the handlers' stack in a bf16 host dtype does."""
    P, N, L, S = _check_maps(maps, item, start, end)
    maps = maps.contiguous()
    rows = end - start
    with torch.cuda.device(maps.device):
        calc = torch.empty(rows, S, dtype=torch.float32, device=maps.device)
        energy = torch.empty_like(calc)
        ws = _workspace(P, rows, S, 1, maps.device)
        native.check(native.lib().ace355_align_timestamp_matrix(native.ptr(maps), P, N, L, S, item, start, rows, float(violence_level),
                                                                int(medfilt_width), _round_flag(dtype), native.ptr(calc), native.ptr(energy),
                                                                native.ptr(ws), ws.numel(), native.current_stream_ptr()),
                     "align_timestamp_matrix")
    return calc, energy


def score_matrix(maps: torch.Tensor, item: int, start: int, end: int, medfilt_width: int = 1, dtype=torch.float32
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``MusicLyricScorer._preprocess_attention``: (calc, energy), fp32 [rows, S]; calc = energy ** 2."""
    P, N, L, S = _check_maps(maps, item, start, end)
    maps = maps.contiguous()
    rows = end - start
    with torch.cuda.device(maps.device):
        calc = torch.empty(rows, S, dtype=torch.float32, device=maps.device)
        energy = torch.empty_like(calc)
        ws = _workspace(P, rows, S, 1, maps.device)
        native.check(native.lib().ace355_align_score_matrix(native.ptr(maps), P, N, L, S, item, start, rows, int(medfilt_width),
                                                            _round_flag(dtype), native.ptr(calc), native.ptr(energy), native.ptr(ws),
                                                            ws.numel(), native.current_stream_ptr()), "align_score_matrix")
    return calc, energy


def dtw_raw(cost_like: torch.Tensor, sign: float = -1.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The DTW of ``sign * cost_like`` for a batch [B, R, S] (or one [R, S]) without a synchronisation: (path int32 [B, 2, R + S],
    right-aligned; path_len int32 [B]; token_frames int32 [B, R, 2], -1 for a row the path skips)."""
    m = cost_like if cost_like.dim() == 3 else cost_like[None]
    if m.dim() != 3 or m.dtype != torch.float32 or not m.is_cuda:
        raise ValueError("dtw wants fp32 device matrices [B, R, S] or [R, S]")
    m = m.contiguous()
    B, R, S = m.shape
    with torch.cuda.device(m.device):
        path = torch.zeros(B, 2, R + S, dtype=torch.int32, device=m.device)
        plen = torch.zeros(B, dtype=torch.int32, device=m.device)
        frames = torch.empty(B, R, 2, dtype=torch.int32, device=m.device)
        ws = _workspace(1, R, S, B, m.device)
        native.check(native.lib().ace355_align_dtw(native.ptr(m), B, R, S, float(sign), native.ptr(path), native.ptr(plen), native.ptr(frames),
                                                   native.ptr(ws), ws.numel(), native.current_stream_ptr()), "align_dtw")
    return path, plen, frames


def dtw(cost_like: torch.Tensor, sign: float = -1.0):
    """``dtw_cpu(sign * cost_like)`` for one matrix [R, S]: (text_idx, time_idx, token_frames) as device tensors, the path trimmed to its
    length (one synchronisation).  A batch [B, R, S] gives a list of such triples."""
    path, plen, frames = dtw_raw(cost_like, sign)
    lens = plen.tolist()
    out = [(path[b, 0, path.shape[-1] - n:], path[b, 1, path.shape[-1] - n:], frames[b]) for b, n in enumerate(lens)]
    return out[0] if cost_like.dim() == 2 else out


def score_metrics(energy: torch.Tensor, path, type_mask, time_weight: float = 0.01, overlap_frames: float = 9.0,
                  instrumental_weight: float = 1.0) -> torch.Tensor:
    """``MusicLyricScorer._compute_alignment_metrics`` in fp64: energy fp32 [B, R, S] or [R, S]; ``path`` either the (path, path_len) pair
    of ``dtw_raw`` or one [len, 2] int tensor of (row, frame) steps (the reference's
    ``path_coords``); type_mask int [R].  Returns fp64 [B, 3] (or [3]) on the device: coverage, monotonicity, path confidence."""
    e = energy if energy.dim() == 3 else energy[None]
    if e.dim() != 3 or e.dtype != torch.float32 or not e.is_cuda:
        raise ValueError("score_metrics wants fp32 device energy [B, R, S] or [R, S]")
    e = e.contiguous()
    B, R, S = e.shape
    dev = e.device
    if isinstance(path, (tuple, list)):
        pth, plen = path
    else:
        p = torch.as_tensor(path).to(device=dev, dtype=torch.int32)
        if p.dim() != 2 or p.shape[1] != 2:
            raise ValueError("path must be [len, 2]")
        p = p.t()
        n = p.shape[1]
        if n > R + S:
            raise ValueError("a path is at most R + S steps long")
        pth = torch.zeros(B, 2, R + S, dtype=torch.int32, device=dev)
        pth[:, :, R + S - n:] = p
        plen = torch.full((B,), n, dtype=torch.int32, device=dev)
    if tuple(pth.shape) != (B, 2, R + S) or tuple(plen.shape) != (B,):
        raise ValueError("path / path_len do not fit the energy batch")
    mask = torch.as_tensor(type_mask).to(device=dev, dtype=torch.int32).contiguous()
    if tuple(mask.shape) != (R,):
        raise ValueError("type_mask must have one entry per row")
    with torch.cuda.device(dev):
        out = torch.empty(B, 3, dtype=torch.float64, device=dev)
        ws = _workspace(1, R, S, B, dev)
        native.check(native.lib().ace355_align_score_metrics(native.ptr(e), native.ptr(pth.contiguous()), native.ptr(plen.contiguous()),
                                                             native.ptr(mask), B, R, S, float(time_weight), float(overlap_frames),
                                                             float(instrumental_weight), native.ptr(out), native.ptr(ws), ws.numel(),
                                                             native.current_stream_ptr()), "align_score_metrics")
    return out if energy.dim() == 3 else out[0]


def median(x: torch.Tensor, dim: int) -> torch.Tensor:
    """``torch.quantile(x, 0.5, dim)`` through the selection the matrices use (``ace355_align_median``); fp32 device tensor."""
    if x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError("median wants an fp32 device tensor")
    dim = dim % x.dim()
    x = x.contiguous()
    outer = 1
    for d in x.shape[:dim]:
        outer *= d
    inner = 1
    for d in x.shape[dim + 1:]:
        inner *= d
    with torch.cuda.device(x.device):
        out = torch.empty(x.shape[:dim] + x.shape[dim + 1:], dtype=torch.float32, device=x.device)
        native.check(native.lib().ace355_align_median(native.ptr(x), outer, x.shape[dim], inner, native.ptr(out), native.current_stream_ptr()),
                     "align_median")
    return out


def final_score(coverage: float, monotonicity: float, confidence: float) -> float:
    """``calculate_score``: clip(cov^2 mono^2 conf, 0, 1) to 4 places."""
    return round(float(min(1.0, max(0.0, (coverage ** 2) * (monotonicity ** 2) * confidence))), 4)


# ------------------------------------------------------------------------------------------------------------------ host-side text
@dataclass
class TokenTimestamp:
    token_id: int
    text: str
    start: float
    end: float
    probability: float


@dataclass
class SentenceTimestamp:
    text: str
    start: float
    end: float
    tokens: List[TokenTimestamp]
    confidence: float


def payload_types():
    """The host's ``TokenTimestamp`` / ``SentenceTimestamp`` when ``acestep.core.scoring.dit_alignment`` imports, else this package's."""
    try:
        from acestep.core.scoring.dit_alignment import SentenceTimestamp as S, TokenTimestamp as T
        return T, S
    except Exception:
        return TokenTimestamp, SentenceTimestamp


def token_type_mask(tokenizer, ids: Sequence[int]) -> List[int]:
    """1 for a lyric token, 0 for every token from one whose text holds "[" up to and including the next whose text holds "]"."""
    mask, inside = [], False
    for tid in ids:
        text = tokenizer.decode([tid])
        inside = inside or "[" in text
        closes = "]" in text
        mask.append(0 if inside or closes else 1)
        if closes:
            inside = False
    return mask


def decode_tokens_incrementally(tokenizer, ids: Sequence[int]) -> List[str]:
    """Each token's own text as the bytes it adds to the decode of the prefix, so a multi-byte character split over byte-level tokens
    lands whole on the token that completes it; "" for a token that adds no complete character (or shortens the decode)."""
    out, seen = [], b""
    ids = list(ids)
    for i in range(len(ids)):
        now = tokenizer.decode(ids[:i + 1], skip_special_tokens=False).encode("utf-8", errors="surrogatepass")
        piece = ""
        if len(now) >= len(seen):
            try:
                piece = now[len(seen):].decode("utf-8")
            except UnicodeDecodeError:
                piece = ""
        out.append(piece)
        seen = now
    return out


def token_timestamps(tokenizer, ids: Sequence[int], token_frames: Sequence[Sequence[int]], n_frames: int, total_duration_seconds: float,
                     token_type=None) -> list:
    """Seconds from the first / last frame of each token on the path (``token_frames[i] = (first, last)``, first < 0: not on the path; such
    a token starts and ends where the previous one ended, 0.0 at the front)."""
    T = token_type or payload_types()[0]
    spf = total_duration_seconds / n_frames
    texts = decode_tokens_incrementally(tokenizer, ids)
    out = []
    for i, tid in enumerate(ids):
        first, last = int(token_frames[i][0]), int(token_frames[i][1])
        if first < 0:
            start = out[-1].end if out else 0.0
            end = start
        else:
            start, end = first * spf, last * spf
        out.append(T(token_id=tid, text=texts[i], start=float(start), end=float(max(end, start)), probability=0.0))
    return out


def sentence_timestamps(tokenizer, tokens: list, sentence_type=None) -> list:
    """Sentences end at a token whose text holds a newline; blank ones are dropped.  Confidence: the mean of the positive token
    probabilities, min-max normalised over the sentences when they differ, 2 places."""
    S = sentence_type or payload_types()[1]
    out, run = [], []

    def close():
        text = tokenizer.decode([t.token_id for t in run], skip_special_tokens=False).strip()
        if text:
            pos = [t.probability for t in run if t.probability > 0]
            out.append(S(text=text, start=round(run[0].start, 3), end=round(run[-1].end, 3), tokens=list(run),
                         confidence=sum(pos) / len(pos) if pos else 0.0))
    for tok in tokens:
        run.append(tok)
        if "\n" in tok.text:
            close()
            run = []
    if run:
        close()
    if out:
        lo, hi = min(s.confidence for s in out), max(s.confidence for s in out)
        for s in out:
            s.confidence = round((s.confidence - lo) / (hi - lo), 2) if hi - lo > 1e-9 else round(s.confidence, 2)
    return out


def format_lrc(sentences: list) -> str:
    """One ``[mm:ss.xx]text`` line per sentence."""
    return "\n".join(f"[{int(s.start // 60):02d}:{s.start % 60:05.2f}]{s.text}" for s in sentences)


# ------------------------------------------------------------------------------------------------------------------ whole stages
def timestamp_spans(maps: torch.Tensor, item: int, start: int, end: int, dtype=torch.float32, violence_level: float = 2.0,
                    medfilt_width: int = 1) -> List[List[int]]:
    """maps -> consensus matrix -> DTW on the device, then one synchronisation: the (first, last) frame of each lyric row on the path."""
    calc, _ = timestamp_matrix(maps, item, start, end, violence_level, medfilt_width, dtype)
    _, _, frames = dtw_raw(calc, -1.0)
    return frames[0].cpu().tolist()


def lyric_timestamps(maps: torch.Tensor, item: int, start: int, end: int, tokenizer, ids: Sequence[int], total_duration_seconds: float,
                     dtype=torch.float32, violence_level: float = 2.0, medfilt_width: int = 1) -> Dict[str, Any]:
    """``timestamp_spans``, then the text: token / sentence timestamps and LRC lines."""
    spans = timestamp_spans(maps, item, start, end, dtype, violence_level, medfilt_width)
    toks = token_timestamps(tokenizer, list(ids), spans, maps.shape[-1], total_duration_seconds)
    sents = sentence_timestamps(tokenizer, toks)
    return {"token_timestamps": toks, "sentence_timestamps": sents, "lrc_text": format_lrc(sents)}


def lyric_scores(maps: torch.Tensor, items: Sequence[int], start: int, end: int, tokenizer, ids: Sequence[int], dtype=torch.float32,
                 medfilt_width: int = 1) -> List[float]:
    """The lyric score of each item of ``items`` (the (lm, dit) pair of a score call): their score matrices go through the DTW and the
    metrics as one batch.  One synchronisation: the [len(items), 3] metrics."""
    mask = token_type_mask(tokenizer, list(ids))
    if len(mask) != end - start:
        mask = [1] * (end - start)
    return [final_score(*m) for m in score_metric_values(maps, items, start, end, mask, dtype, medfilt_width)]


def score_metric_values(maps: torch.Tensor, items: Sequence[int], start: int, end: int, mask: Sequence[int], dtype=torch.float32,
                        medfilt_width: int = 1) -> List[List[float]]:
    """maps -> score matrices -> one DTW batch -> metrics on the device, then one synchronisation: [coverage, monotonicity, confidence]
    per item."""
    mats = [score_matrix(maps, it, start, end, medfilt_width, dtype) for it in items]
    calc = torch.stack([c for c, _ in mats])
    energy = torch.stack([e for _, e in mats])
    path, plen, _ = dtw_raw(calc, -1.0)
    return score_metrics(energy, (path, plen), torch.tensor(list(mask), dtype=torch.int32)).cpu().tolist()
