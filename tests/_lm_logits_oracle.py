"""numpy fp32 restatement of the 5 Hz LM's logits stage (include/ace355.h above ``ace355_lm_shape``), and the G23 fixture's layout.

The five steps, each a separate numpy fp32 operation (numpy never fuses), are what the reference computes with separate torch kernels:
the CFG combine (llm_inference.py:2482), ``MetadataConstrainedLogitsProcessor.__call__``'s mask, EOS rule and temperature
(constrained_logits_processor.py:1583-1629, 1666-1695), transformers' ``RepetitionPenaltyLogitsProcessor``.  G23 records the reference's
own output for every case; tests/test_lm_logits_cpu.py holds this file to it bit for bit.
"""
import os

import numpy as np

G23 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_lm_logits.npz")
EOS_NONE, EOS_BLOCK, EOS_FORCE = 0, 1, 2
# the processor branch a fixture setting ran: name -> (which recorded mask is added, EOS rule)
MODES = {"none": ("codes", EOS_NONE), "block": ("codes", EOS_BLOCK), "force": ("codes", EOS_FORCE), "disabled": (None, EOS_NONE),
         "understand": ("audio", EOS_NONE), "completed": (None, EOS_NONE)}
MODE_NAMES = list(MODES)
CFG_SCALE = 1.7
MIN_T = 1e-6


def seen_bitmap(ids, V):
    """uint32 [B, ceil(V / 32)]: bit v & 31 of word v >> 5 for every id of the row inside [0, V)."""
    ids = np.asarray(ids, dtype=np.int64)
    if ids.ndim == 1:
        ids = ids[:, None]
    out = np.zeros((ids.shape[0], (V + 31) // 32), dtype=np.uint32)
    for b in range(ids.shape[0]):
        for v in ids[b]:
            if 0 <= v < V:
                out[b, v >> 5] |= np.uint32(1) << np.uint32(v & 31)
    return out


def seen_bool(seen, V):
    """[B, V] bool from the bitmap."""
    v = np.arange(V)
    return ((np.asarray(seen, dtype=np.uint32)[:, v >> 5] >> (v & 31).astype(np.uint32)) & 1).astype(bool)


def shape(cond, uncond=None, cfg_scale=1.0, mask=None, eos_id=None, eos_mode=EOS_NONE, temperature=None, penalty=1.0, seen=None):
    """fp32 [B, V].  ``temperature`` None: no division; <= 0: 1e-6.  ``seen``: the uint32 bitmap (needed iff penalty != 1)."""
    f = np.float32
    with np.errstate(all="ignore"):
        c = np.asarray(cond, dtype=f)
        V = c.shape[1]
        if uncond is None:
            x = c.copy()
        else:
            u = np.asarray(uncond, dtype=f)
            x = u + f(cfg_scale) * (c - u)
        if mask is not None:
            x = x + np.asarray(mask, dtype=f)[None, :]
        if eos_mode == EOS_BLOCK:
            x[:, eos_id] = -np.inf
        elif eos_mode == EOS_FORCE:
            keep = x[:, eos_id].copy()
            x[:] = -np.inf
            x[:, eos_id] = keep
        if temperature is not None:
            x = x / f(temperature if temperature > 0 else MIN_T)
        if penalty != 1.0:
            hit = seen_bool(seen, V)
            x = np.where(hit, np.where(x < 0, x * f(penalty), x / f(penalty)), x)
        return x.astype(f)


def same_bits(a, b):
    """Bit equality of two fp32 arrays, NaN compared by position (any NaN payload equals any other)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.uint32)[~na] == b.view(np.uint32)[~nb]).all())


def load_g23_stage():
    """[(cond, uncond, masks {"codes", "audio"}, eos_id, history ids, [(mode name, T or None, penalty, expected)])] per case."""
    z = np.load(G23)
    cases = []
    for c in range(int(z["n_stage"])):
        sets = []
        for s in range(len(z[f"s{c}_mode"])):
            T = float(z[f"s{c}_T"][s])
            sets.append((MODE_NAMES[int(z[f"s{c}_mode"][s])], None if np.isnan(T) else T, float(z[f"s{c}_pen"][s]), z[f"s{c}_out{s}"]))
        cases.append((z[f"s{c}_cond"], z[f"s{c}_uncond"], {"codes": z[f"s{c}_mask"], "audio": z[f"s{c}_amask"]}, int(z[f"s{c}_eos"]),
                      z[f"s{c}_hist"], sets))
    return cases


def expected_for(case, setting):
    """The oracle's output for one recorded setting of one case."""
    cond, uncond, masks, eos, hist, _sets = case
    mode, T, pen, _want = setting
    which, eos_mode = MODES[mode]
    return shape(cond, uncond, CFG_SCALE, masks[which] if which else None, eos, eos_mode, T, pen, seen_bitmap(hist, cond.shape[1]))
