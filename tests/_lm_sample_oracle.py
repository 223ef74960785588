"""fp64 numpy restatement of the LM token selection (include/ace355.h above ``ace355_lm_pick``): keep mask, kept count, greedy token,
the CDF over ascending ids and the token for a given fp32 ``u``.  One row at a time; ``p``, ``T`` and ``u`` are taken through fp32, as the
C ABI carries them.  Shared by the CPU and GPU tests and by tests/golden/make_g22_lm_sample.py."""
import os

import numpy as np

G22 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_lm_sample.npz")
SETTINGS = 4   # per G22 case: (k off, p 0.9), (k, p off), (k, p 0.95), (both off)


def is_bad(x):
    x = np.asarray(x, dtype=np.float32)
    return bool(np.isnan(x).any() or np.isposinf(x).any() or not np.isfinite(x).any())


def _walk(x, k):
    """Survivors of top-k, and the descending walk over them: (survivor mask, order of survivor ids, masses in that order, Z)."""
    x = np.asarray(x, dtype=np.float32)
    V = x.shape[0]
    xs = x.astype(np.float64) + 0.0   # (-0.0 + 0.0 == +0.0)
    surv = np.ones(V, dtype=bool)
    if k is not None and 0 < k < V:
        t = np.sort(xs)[::-1][k - 1]
        surv = xs >= t
    ids = np.nonzero(surv)[0]
    order = ids[np.lexsort((ids, -xs[ids]))]   # descending value, equal values in ascending id
    with np.errstate(invalid="ignore"):
        m = np.where(np.isneginf(xs[order]), 0.0, np.exp(xs[order] - xs.max()))
    return surv, order, m, float(m.sum())


def keep_mask(x, k=None, p=None):
    """bool [V]: finite, survives top-k (0 < k < V) and top-p (0 < p < 1).  All False for a bad row."""
    x = np.asarray(x, dtype=np.float32)
    if is_bad(x):
        return np.zeros(x.shape[0], dtype=bool)
    surv, order, m, Z = _walk(x, k)
    keep = surv.copy()
    if p is not None and 0.0 < p < 1.0:
        before = np.concatenate([[0.0], np.cumsum(m)[:-1]])
        kept_pos = before / Z <= np.float64(np.float32(p))
        kept_pos[0] = True
        keep = np.zeros(x.shape[0], dtype=bool)
        keep[order[kept_pos]] = True
    return keep & np.isfinite(x)


def top_p_margin(x, k, p):
    """(distance of the nearest prefix mass from p, over every position j >= 1 of the walk; whether the values either side of the cut
    differ).  (inf, True) when top-p is off or the walk has one position."""
    x = np.asarray(x, dtype=np.float32)
    if p is None or not 0.0 < p < 1.0 or is_bad(x):
        return float("inf"), True
    _surv, order, m, Z = _walk(x, k)
    if order.shape[0] < 2:
        return float("inf"), True
    before = np.cumsum(m)[:-1] / Z
    p32 = np.float64(np.float32(p))
    n_kept = 1 + int((before <= p32).sum())
    differ = n_kept >= order.shape[0] or x[order[n_kept - 1]] != x[order[n_kept]]
    return float(np.abs(before - p32).min()), bool(differ)


def greedy_token(x, keep):
    if not keep.any():
        return -1
    xs = np.where(keep, np.asarray(x, dtype=np.float64), -np.inf)
    return int(np.argmax(xs))   # (the first position of the maximum)


def cdf(x, keep, T):
    """(kept ids ascending, their weights exp((x - max) / T), the running sum over them)."""
    ids = np.nonzero(keep)[0]
    xs = np.asarray(x, dtype=np.float32).astype(np.float64)
    w = np.exp((xs[ids] - xs.max()) / np.float64(np.float32(T)))
    return ids, w, np.cumsum(w)


def token_for_u(x, keep, T, u):
    """The first kept id whose running weight sum exceeds u * W, else the last kept id with a non-zero weight; -1 for an empty mask."""
    if not keep.any():
        return -1
    if not T > 0:
        return greedy_token(x, keep)
    ids, w, c = cdf(x, keep, T)
    hit = np.nonzero(c > np.float64(np.float32(u)) * c[-1])[0]
    if hit.shape[0]:
        return int(ids[hit[0]])
    return int(ids[np.nonzero(w > 0)[0][-1]])


def load_g22():
    """[(x float32 [R, V], [(k, p, finite bool [R, V], greedy int64 [R]) per setting])] per case."""
    z = np.load(G22)
    out = []
    for c in range(int(z["n_cases"])):
        x = z[f"c{c}_x"]
        sets = []
        for s in range(SETTINGS):
            k, p = int(z[f"c{c}_k"][s]), float(z[f"c{c}_p"][s])
            fin = np.unpackbits(z[f"c{c}_s{s}_finite"], axis=1, count=x.shape[1]).astype(bool)
            sets.append((k if k > 0 else None, p if p > 0 else None, fin, z[f"c{c}_s{s}_greedy"]))
        out.append((x, sets))
    return out
