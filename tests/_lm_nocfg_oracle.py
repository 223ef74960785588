"""numpy restatement of the 5 Hz LM's logits stage in bf16 (include/ace355.h above ``ace355_lm_shape_as``), and the G26 fixture's
stage layout.

The fp32 oracle's operations (tests/_lm_logits_oracle.py) with ``r()`` between them: ``r`` is round-to-nearest-even of an fp32 value
to bf16, kept in fp32, done on the uint32 bit pattern.  That is what torch on the CPU computes when the reference's non-CFG loop
(llm_inference.py:2369-2377) hands bf16 logits to ``MetadataConstrainedLogitsProcessor.__call__`` and transformers'
``RepetitionPenaltyLogitsProcessor``: every kernel computes in fp32 and rounds its result to bf16.  G26 records the reference's own
output for every case; tests/test_lm_nocfg_cpu.py holds this file to it bit for bit.
"""
import os

import numpy as np

import _lm_logits_oracle as O

G26 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g26_lm_nocfg.npz")
STAGE_V = (1, 31, 32, 33, 65, 1003, 2051)
TEMPS = (None, 0.7, 0.6, 0.0)
PENS = (1.0, 1.1, 1.3)


def rne(x):
    """fp32 array -> the nearest bf16 value (ties to even) as fp32.  NaN stays NaN, +-inf and +-0 stay, subnormals round like any
    value, a finite value past bf16's largest becomes inf."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32)
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = (b.astype(np.uint64) + np.uint64(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1)).astype(np.uint64)).astype(np.uint32)
    r &= np.uint32(0xFFFF0000)
    r = np.where(nan, (b & np.uint32(0x80000000)) | np.uint32(0x7FC00000), r).astype(np.uint32)
    return r.view(np.float32).reshape(x.shape)


def is_bf16(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    return bool(((x.view(np.uint32) & np.uint32(0xFFFF)) == 0)[~np.isnan(x)].all())


def shape(cond, mask=None, eos_id=None, eos_mode=O.EOS_NONE, temperature=None, penalty=1.0, seen=None):
    """fp32 [B, V] of bf16-representable values.  Arguments as ``_lm_logits_oracle.shape`` without the CFG pair."""
    f = np.float32
    with np.errstate(all="ignore"):
        x = rne(np.asarray(cond, dtype=f))
        V = x.shape[1]
        if mask is not None:
            x = rne(x + rne(np.asarray(mask, dtype=f))[None, :])
        if eos_mode == O.EOS_BLOCK:
            x[:, eos_id] = -np.inf
        elif eos_mode == O.EOS_FORCE:
            keep = x[:, eos_id].copy()
            x[:] = -np.inf
            x[:, eos_id] = keep
        if temperature is not None:
            x = rne(x / f(temperature if temperature > 0 else O.MIN_T))
        if penalty != 1.0:
            hit = O.seen_bool(seen, V)
            x = np.where(hit, np.where(x < 0, rne(x * f(penalty)), rne(x / f(penalty))), x)
        return x.astype(f)


def shape_as(cond, dtype, **kw):
    """The stage at either dtype: "bf16" is ``shape`` above, "fp32" the fp32 oracle without a CFG pair."""
    if dtype == "bf16":
        return shape(cond, **kw)
    return O.shape(cond, None, 1.0, kw.get("mask"), kw.get("eos_id"), kw.get("eos_mode", O.EOS_NONE), kw.get("temperature"),
                   kw.get("penalty", 1.0), kw.get("seen"))


def halfway_mask(x, T):
    """Which elements of the bf16-valued ``x`` have an fp32 quotient ``x / T`` exactly half-way between two bf16 neighbours."""
    with np.errstate(all="ignore"):
        q = (np.asarray(x, dtype=np.float32) / np.float32(T)).astype(np.float32)
    return np.isfinite(q) & ((q.view(np.uint32) & np.uint32(0xFFFF)) == np.uint32(0x8000))


def stage_settings(V):
    """(mode, T, penalty) per case, thinned for the large V as G23 thins them."""
    if V <= 65:
        return [(m, T, p) for m in O.MODE_NAMES for T in TEMPS for p in PENS]
    if V == 1003:
        return [(m, T, p) for m in O.MODE_NAMES for T, p in ((None, 1.0), (0.7, 1.1), (0.0, 1.3), (0.6, 1.3), (0.6, 1.0))]
    return [(m, TEMPS[i % 4], (1.3, 1.0, 1.1)[i % 3]) for i, m in enumerate(O.MODE_NAMES)]


def load_g26_stage():
    """[(logits (bf16-valued fp32), masks {"codes", "audio"}, eos_id, history ids, [(mode, T or None, penalty, expected)])] per case."""
    z = np.load(G26)
    cases = []
    for c in range(int(z["n_stage"])):
        sets = []
        for s in range(len(z[f"s{c}_mode"])):
            T = float(z[f"s{c}_T"][s])
            sets.append((O.MODE_NAMES[int(z[f"s{c}_mode"][s])], None if np.isnan(T) else T, float(z[f"s{c}_pen"][s]), z[f"s{c}_out{s}"]))
        cases.append((z[f"s{c}_cond"], {"codes": z[f"s{c}_mask"], "audio": z[f"s{c}_amask"]}, int(z[f"s{c}_eos"]), z[f"s{c}_hist"], sets))
    return cases


def expected_for(case, setting):
    cond, masks, eos, hist, _sets = case
    mode, T, pen, _want = setting
    which, eos_mode = O.MODES[mode]
    return shape(cond, masks[which] if which else None, eos, eos_mode, T, pen, O.seen_bitmap(hist, cond.shape[1]))
