"""Attention, weight by weight: read the softmax matrix P back through a one-hot V and hold every element to a derived bound (helper
module, no tests here; tests/test_attn_keys_cpu.py and tests/test_attention_keys_gpu.py use it).

out = P V, so a V whose rows are distinct unit vectors makes the output the probability matrix itself.  A case runs ceil(Skv / 128)
launches; in run r, key j of [128 r, 128 r + 128) has the single non-zero entry

    V[n, j, g * 128 + perm(j - 128 r)] = 2^(g mod 4 + 4 (n mod 2)),        g the KV head,

and every other key is all zero.  Then out[n, i, h * 128 + perm(j - 128 r)] / 2^(...) = p[n, h, i, j]: one softmax weight per output
element, untouched by the fp32 accumulation of exact zeros.  perm(x) = (5 x + 3) mod 128 is a permutation that is not an involution (a
V / V^T mix-up or a permutation of the head dim would hide behind a symmetric pattern); the powers of two are exact in bf16 and turn a
read of the wrong KV head's or the wrong sequence's V into a factor.

The reference is fp64 torch from the same bf16 q, k, with the visibility written from its definition: |i - j| <= window when window >= 0,
j < kv_len[n] when masked; a row without a visible key (masked cases only) is uniform 1 / Skv over ALL keys (oracle/cond.mask_4d; AttnArgs::
vmean in csrc/common.h).  Nothing here knows about key tiles, query blocks or split parts.

The bound, for every element of every run (compare):
  1. reference weight 0 (invisible key):  got == 0 exactly;
  2. reference weight p > 0:              |got - p| <= (2 U + U^2 + 2^-12) p, U = 2^-8: P is rounded to bf16 before P V, the quotient
     is rounded to bf16 (round to nearest even), l is an fp32 sum of the unrounded p; 2^-12 covers v_exp_f32, the fp32 score sum and
     the merges' fp32 arithmetic (each at or below 1e-5 relative at these score ranges);
  3. reference weight p > 0:              got > 0 (the caller asserts that the smallest such p is far above the bf16 / fp32 underflow);
  4. output columns no key of the run's block maps to (a short last block): exactly 0.
Nothing runs on a device unless the caller's tensors live on one.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from _vae_layers import U_BF16 as U

Tensor = torch.Tensor
Shape = Tuple[int, int, int, int, int, int]   # (N, Sq, Skv, Hq, Hkv, window)

BLOCK = 128                                  # keys read back per run = the head dim
REL_BOUND = 2 * U + U * U + 2.0 ** -12
P_FLOOR = 2.0 ** -60                          # the smallest visible reference weight a case may have (fp32 / bf16 normal range: 2^-126)
SCALE = 128 ** -0.5


def perm(x):
    return (5 * x + 3) % BLOCK


def n_runs(Skv: int) -> int:
    return -(-Skv // BLOCK)


def v_weight(N: int, Hkv: int) -> Tensor:
    """[N, Hkv] fp32: the value a key's one-hot entry carries, 2^(g mod 4 + 4 (n mod 2))."""
    n, g = torch.arange(N)[:, None], torch.arange(Hkv)[None, :]
    return torch.pow(2.0, (g % 4 + 4 * (n % 2)).float())


def one_hot_v(shape: Shape, r: int) -> Tensor:
    """V of run r, bf16 [N, Skv, Hkv * 128]."""
    N, _Sq, Skv, _Hq, Hkv, _w = shape
    v = torch.zeros(N, Skv, Hkv, BLOCK)
    j = torch.arange(BLOCK * r, min(Skv, BLOCK * r + BLOCK))
    v[:, j, :, perm(j - BLOCK * r)] = v_weight(N, Hkv)[None]   # (the two index vectors lead the indexed shape: [keys, N, Hkv])
    return v.reshape(N, Skv, Hkv * BLOCK).to(torch.bfloat16)


def make_qk(shape: Shape, seed: int, lens: Optional[Sequence[int]] = None) -> Tuple[Tensor, Tensor, Optional[Tuple[int, int, int, int]]]:
    """q [N, Sq, Hq * 128], k [N, Skv, Hkv * 128]: randn rounded to bf16, different for every (n, head), and the (n, h, i, j) of the key
    spike written into k - tests/test_kernels_gpu.py::test_attention_rescale_branch's k[j] = 3 q[i], None when the case has a single key.
    j is the LAST key visible to query i (for full attention the last key of the ragged tail), and i is chosen so that j lies in a later
    64-key tile than the row's first visible key: the running max moves late, by far more than the deferred-rescale threshold.  The
    spike's score is 3 |q_i|^2 / sqrt(128), about 34 +- 4, and the row's other weights fall by that much: of the 16 rows that qualify,
    i is the one with the smallest |q_i|, which keeps them above P_FLOOR.  The last sequence (the last of full length when masked), the
    last head."""
    N, Sq, Skv, Hq, Hkv, window = shape
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(N, Sq, Hq * BLOCK, generator=g).to(torch.bfloat16)
    k = torch.randn(N, Skv, Hkv * BLOCK, generator=g).to(torch.bfloat16)
    if Skv < 2:
        return q, k, None
    n = N - 1 if lens is None else max(i for i, length in enumerate(lens) if length == Skv)
    h = Hq - 1
    lo = 0 if (window < 0 or window >= 64) else 64 - window
    rows = torch.arange(min(lo, Sq - 1), min(lo + 16, Sq))
    i = int(rows[q[n, rows, h * BLOCK:(h + 1) * BLOCK].float().pow(2).sum(1).argmin()])
    j = Skv - 1 if window < 0 else min(Skv - 1, i + window)
    kvh = h // (Hq // Hkv)
    k[n, j, kvh * BLOCK:(kvh + 1) * BLOCK] = (3.0 * q[n, i, h * BLOCK:(h + 1) * BLOCK].float()).to(torch.bfloat16)
    return q, k, (n, h, i, j)


def visibility(Sq: int, Skv: int, window: int, kv_len: Optional[int], device=None) -> Tensor:
    """bool [Sq, Skv], from the definition."""
    i = torch.arange(Sq, device=device)[:, None]
    j = torch.arange(Skv, device=device)[None, :]
    vis = torch.ones(Sq, Skv, dtype=torch.bool, device=device)
    if window >= 0:
        vis &= (i - j).abs() <= window
    if kv_len is not None:
        vis &= j < kv_len
    return vis


def all_pairs(shape: Shape) -> List[Tuple[int, int]]:
    return [(n, h) for n in range(shape[0]) for h in range(shape[3])]


def reference(q: Tensor, k: Tensor, shape: Shape, lens: Optional[Sequence[int]], pairs: Sequence[Tuple[int, int]]) -> Tuple[Tensor, Tensor]:
    """(P fp64 [len(pairs), Sq, Skv], visible bool [len(pairs), Sq, Skv]) on q's device, one sequence at a time.  `visible` is the
    definition's; a row without a visible key has P = 1 / Skv on every key."""
    N, Sq, Skv, Hq, Hkv, window = shape
    grp = Hq // Hkv
    q64 = q.double().view(N, Sq, Hq, BLOCK)
    k64 = k.double().view(N, Skv, Hkv, BLOCK)
    P = torch.empty(len(pairs), Sq, Skv, dtype=torch.float64, device=q.device)
    V = torch.empty(len(pairs), Sq, Skv, dtype=torch.bool, device=q.device)
    for n in sorted({n for n, _h in pairs}):
        vis = visibility(Sq, Skv, window, None if lens is None else int(lens[n]), q.device)
        dead = ~vis.any(1)
        for at, (n2, h) in enumerate(pairs):
            if n2 != n:
                continue
            s = (q64[n, :, h] @ k64[n, :, h // grp].t()) * SCALE
            s = s.masked_fill(~vis, float("-inf"))
            s[dead] = 0.0                      # no visible key: uniform over all keys
            P[at] = torch.softmax(s, dim=1)
            V[at] = vis
    return P, V


def decode(out: Tensor, shape: Shape, r: int) -> Tuple[Tensor, Tensor]:
    """out bf16 [N, Sq, Hq * 128] of run r -> (the weights of the run's keys, fp32 [N, Hq, Sq, width] - exact: a bf16 value over a power
    of two -, the output columns no key maps to, [N, Hq, Sq, 128 - width])."""
    N, Sq, Skv, Hq, Hkv, _w = shape
    width = min(BLOCK, Skv - BLOCK * r)
    o = out.float().view(N, Sq, Hq, BLOCK).permute(0, 2, 1, 3)
    cols = perm(torch.arange(BLOCK, device=out.device))
    wt = v_weight(N, Hkv).to(out.device).repeat_interleave(Hq // Hkv, dim=1)[:, :, None, None]
    return o[..., cols[:width]] / wt, o[..., cols[width:]]


def compare(got: Tensor, stray: Tensor, want: Tensor, visible: Tensor, pairs: Sequence[Tuple[int, int]], j0: int, label: str = "",
            max_lines: int = 8) -> Dict[str, object]:
    """One run: got [N, Hq, Sq, width] and stray [N, Hq, Sq, 128 - width] from decode, want / visible [len(pairs), Sq, width] the
    reference's columns j0 .. j0 + width.  The pairs are held to the bound; EVERY (n, h) is held to the zeros the pairs' sequences show
    (visibility does not depend on the head) and to clean stray columns.  Returns the count of broken elements, the largest relative
    error of a weight in units of U and a report of the first offenders: (n, h, i, j, got, want, visible)."""
    dev = got.device
    nn = torch.tensor([n for n, _h in pairs], device=dev)
    hh = torch.tensor([h for _n, h in pairs], device=dev)
    g = got[nn, hh].double()
    zero = want == 0
    err = (g - want).abs()
    bad = torch.where(zero, g != 0, ~((err <= REL_BOUND * want) & (g > 0)))   # (NaN fails either way)
    rel = torch.where(zero, torch.zeros_like(err), err / want.clamp_min(1e-300))
    rel = torch.where(torch.isfinite(rel), rel, torch.full_like(rel, float("inf")))
    lines: List[str] = []
    n_bad = int(bad.sum())
    for at, i, j in bad.nonzero()[:max_lines].tolist():
        lines.append(f"  {label}: n {pairs[at][0]} h {pairs[at][1]} i {i} j {j0 + j}: got {float(g[at, i, j]):.9g} want {float(want[at, i, j]):.9g} "
                     f"visible {bool(visible[at, i, j])} (|got - want| / want = {float(rel[at, i, j]) / U:.3f} U)")
    # every head of a sequence sees the same keys: the zeros of one pair per sequence hold for the heads outside the pairs too
    held = set(pairs)
    for n in sorted({n for n, _h in pairs}):
        at = next(a for a, (n2, _h) in enumerate(pairs) if n2 == n)
        others = [h for h in range(got.shape[1]) if (n, h) not in held]
        if not others:
            continue
        leak = (got[n, others] != 0) & zero[at][None]
        n_bad += int(leak.sum())
        for hi, i, j in leak.nonzero()[:max_lines].tolist():
            lines.append(f"  {label}: n {n} h {others[hi]} i {i} j {j0 + j}: got {float(got[n, others[hi], i, j]):.9g} want 0 visible False")
    dirty = stray != 0
    n_stray = int(dirty.sum())
    for n, h, i, c in dirty.nonzero()[:max_lines].tolist():
        lines.append(f"  {label}: n {n} h {h} i {i}: output column {perm(BLOCK - stray.shape[3] + c)}, which no key of the block maps to, holds "
                     f"{float(stray[n, h, i, c]):.9g}")
    n_bad += n_stray
    if n_bad:
        lines.insert(0, f"{label}: {n_bad} elements break (invisible: got == 0; visible: got > 0 and |got - p| <= {REL_BOUND / U:.4f} U p)")
    pos = want[~zero]
    return {"n_bad": n_bad, "max_err_u": float(rel.max()) / U if rel.numel() else 0.0, "min_p": float(pos.min()) if pos.numel() else 1.0,
            "report": "\n".join(lines[:1 + 3 * max_lines])}


def run_case(shape: Shape, lens: Optional[Sequence[int]], attend: Callable[[Tensor, Tensor, Tensor], Tensor], seed: int = 0,
             pairs: Optional[Sequence[Tuple[int, int]]] = None, device="cpu", label: str = "") -> Dict[str, object]:
    """Every run of one case.  attend(q, k, v) -> out (bf16 [N, Sq, Hq * 128]) on `device` is the code under test; the reference is
    computed once on the same device.  Asserts nothing: returns {"n_bad", "max_err_u", "min_p", "runs", "report"}."""
    _N, _Sq, Skv, _Hq, _Hkv, _w = shape
    pairs = all_pairs(shape) if pairs is None else list(pairs)
    q, k, _spike = make_qk(shape, seed, lens)
    q, k = q.to(device), k.to(device)
    P, vis = reference(q, k, shape, lens, pairs)
    n_bad, worst, min_p, reports = 0, 0.0, 1.0, []
    for r in range(n_runs(Skv)):
        out = attend(q, k, one_hot_v(shape, r).to(device))
        got, stray = decode(out, shape, r)
        j0 = BLOCK * r
        res = compare(got, stray, P[:, :, j0:j0 + got.shape[3]], vis[:, :, j0:j0 + got.shape[3]], pairs, j0, f"{label} run {r}")
        n_bad += res["n_bad"]
        worst, min_p = max(worst, res["max_err_u"]), min(min_p, res["min_p"])
        if res["n_bad"] and len(reports) < 3:
            reports.append(res["report"])
    return {"n_bad": n_bad, "max_err_u": worst, "min_p": min_p, "runs": n_runs(Skv), "report": "\n".join(reports)}


# ------------------------------------------------------------------------------------------------ a torch emulation of the kernels' arithmetic
def _bf16_round(x: Tensor) -> Tensor:
    return x.to(torch.bfloat16).float()


def _bf16_truncate(x: Tensor) -> Tensor:
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def emulate(q: Tensor, k: Tensor, v: Tensor, shape: Shape, lens: Optional[Sequence[int]] = None, *, band_delta: int = 0, pad_leak: bool = False,
            double_last: bool = False, kv_head_mod: bool = False, v_transposed: bool = False, truncate: bool = False, defer: float = 8.0) -> Tensor:
    """The arithmetic of attn.hip in torch, for tests/test_attn_keys_cpu.py: fp32 scores in log2 units, a walk over 64-key tiles with a
    running max that 32 rows move together and only when a tile's max exceeds it by more than `defer` (so p = 2^(s - m) is formed against
    a stale max), p rounded to bf16 ahead of P V, l an fp32 sum of the unrounded p, the quotient rounded to bf16, and the mean of V for a
    row without a key.  Each keyword is one deliberate error the method has to catch."""
    N, Sq, Skv, Hq, Hkv, window = shape
    rnd = _bf16_truncate if truncate else _bf16_round
    grp = Hq // Hkv
    qf = q.float().view(N, Sq, Hq, BLOCK)
    kf = k.float().view(N, Skv, Hkv, BLOCK)
    vf = v.float().view(N, Skv, Hkv, BLOCK)
    out = torch.zeros(N, Sq, Hq, BLOCK)
    scale_log2 = SCALE * 1.4426950408889634
    for n in range(N):
        vis = visibility(Sq, Skv, window + band_delta if window >= 0 else window, None if lens is None else int(lens[n]))
        for h in range(Hq):
            g = h % Hkv if kv_head_mod else h // grp
            kk, vv, vs = kf[n, :, g], vf[n, :, g], vis
            if v_transposed:
                vv = torch.cat([torch.nn.functional.pad(b, (0, 0, 0, BLOCK - b.shape[0])).t()[:b.shape[0]] for b in vv.split(BLOCK)])
            if pad_leak:       # the first pad key of the ragged tail: the clamped read repeats the last key's K row, V^T's pad is zero
                kk, vv, vs = torch.cat([kk, kk[-1:]]), torch.cat([vv, torch.zeros(1, BLOCK)]), torch.cat([vs, torch.ones(Sq, 1, dtype=torch.bool)], 1)
            if double_last:
                kk, vv, vs = torch.cat([kk, kk[-1:]]), torch.cat([vv, vv[-1:]]), torch.cat([vs, vs[:, -1:]], 1)
            s = (qf[n, :, h] @ kk.t()) * scale_log2
            s = s.masked_fill(~vs, float("-inf"))
            m = torch.full((Sq,), float("-inf"))
            l = torch.zeros(Sq)
            o = torch.zeros(Sq, BLOCK)
            for t0 in range(0, s.shape[1], 64):
                st = s[:, t0:t0 + 64]
                m_tile = st.max(1).values
                want_move = (m_tile - m) > defer                                   # (-inf - -inf = NaN: no move)
                move = torch.nn.functional.pad(want_move, (0, -Sq % 32)).view(-1, 32).any(1).repeat_interleave(32)[:Sq]
                m_new = torch.where(move, torch.maximum(m, m_tile), m)
                m_use = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
                alpha = torch.where(move, torch.exp2(m - m_use), torch.ones_like(m))
                p = torch.exp2(st - m_use[:, None])
                l = l * alpha + p.sum(1)
                o = o * alpha[:, None] + rnd(p) @ vv[t0:t0 + 64]
                m = m_new
            res = rnd(o * (1.0 / l)[:, None])
            dead = l == 0
            res[dead] = rnd(vf[n, :, g].sum(0) / Skv)
            out[n, :, h] = res
    return out.reshape(N, Sq, Hq * BLOCK).to(torch.bfloat16)
