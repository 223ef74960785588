"""The DiT pass requests whose plans tests/dit_plan_table.json records, and the evaluator behind tests/test_dit_plan_cpu.py.

    python tests/_dit_plan_cases.py --write     regenerate the table (after a deliberate change of csrc/dit_plan.h)
    python tests/_dit_plan_cases.py --plans     print the table requests' plans of THIS process (its ACE355_* environment) as JSON

A request is (configuration name, T, sequences, fields): the arguments of native.dit_pass_plan.  No GPU is needed: ace355_dit_pass_plan
evaluates the library's pure plan_dit_pass, with the GEMM and attention plans' answers from their own queries.  The table keeps a plan's
facts, how many steps of each kind (GEMMs by path) it has and a SHA-256 over all its steps, each reduced to the fields that differ from a
blank step (STEP_DEFAULTS).  The rows of STEPS_KEPT also keep the steps themselves (all, or those of the layers named; -1: outside the
layers), so that a change shows which launches moved.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "dit_plan_table.json")

# full size, and the two small configurations of the GPU tests (test_dit_gpu.py: TINY; test_zero_row_and_tile64_switches_keep_the_bits)
CONFIGS = {"full": dict(), "tiny": dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, head_dim=128),
           "mid": dict(hidden_size=1024, intermediate_size=3072, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=4)}
BASE_T = {"full": (750, 769), "tiny": (37, 5), "mid": (200, 33)}   # (T, L) of a configuration's rows
STEP_DEFAULTS = {**{k: -1 for k in ("layer", "gate", "nf_split", "nc_rowsq", "next_layer", "gs")}, **{k: None for k in ("src", "dst", "next_proj")}}


def config(name):
    import ace355
    return ace355.DitConfig(**CONFIGS[name])


# rows whose steps the table keeps, by the part of the name behind the configuration: the layers kept, None: all
STEPS_KEPT = {"tiny: 1 songs, CFG, sampler (folded norms)": None, "tiny: 2 songs, CFG, plain forward": None, "tiny: 1 songs, no CFG, sampler": None,
              "tiny: layers 0 and 1 tapped": None, "tiny: maps stopping at a middle layer": None, "mid: metric batch, MXFP8": None,
              "full: 1 songs, CFG, sampler (folded norms)": (-1, 0, 1), "full: metric batch, MXFP8": (-1, 1)}


def cfg_seqs(songs, L, null_L=None):
    """`songs` conditional sequences on slots 0 .. songs - 1, then their CFG copies on the broadcast null slot"""
    return [(b, L, 0) for b in range(songs)] + [(songs, null_L or L, 1)] * songs


def sampler(songs, T, L, fold=True, **fields):
    """a CFG sampler step: one timestep row, schedule tables, both halves with the same inputs"""
    return dict(temb_rows=1, dup_half=1, nf_on=int(fold), nf_emb_on=1, nf_rows=27, nf_cap_M=2 * songs * ((T + 1) // 2), **fields)


def table_requests():
    rows = []
    for name in CONFIGS:
        T, L = BASE_T[name]
        add = lambda what, T_, seqs, fields: rows.append((f"{name}: {what}", name, T_, seqs, fields))
        for songs in (1, 2, 4, 8):
            add(f"{songs} songs, CFG, sampler (folded norms)", T, cfg_seqs(songs, L), sampler(songs, T, L))
            add(f"{songs} songs, CFG, plain forward", T, cfg_seqs(songs, L), {})
            add(f"{songs} songs, no CFG, sampler", T, [(b, L, 0) for b in range(songs)], dict(temb_rows=1, nf_emb_on=1, nf_rows=27))
        add("dual-chain half, 4 songs, 128 CUs", T, cfg_seqs(4, L), sampler(4, T, L, cu_slots=128, prefetch=0))
        add("metric batch, MXFP8", T, cfg_seqs(8, L), dict(temb_rows=1, dup_half=1, nf_emb_on=1, nf_rows=27, precision=1))
        add("metric batch, MXFP8, plain forward", T, cfg_seqs(8, L), dict(precision=1))
        if name == "full":
            add("1 song, CFG, T = 3000", 3000, cfg_seqs(1, L), sampler(1, 3000, L))
            add("1 song, CFG, T = 6000", 6000, cfg_seqs(1, L), sampler(1, 6000, L))
        add("cover switch onto slots of another L (the null slot keeps the cover phase's)", T, cfg_seqs(2, L + 40, null_L=L), sampler(2, T, L))
        add("null slot not broadcast (the generic path)", T, [(0, L, 0), (1, L, 0)], sampler(1, T, L))
        add("two broadcast slots at the end (no shortcut)", T, [(0, L, 0), (1, L, 1), (2, L, 1)], dict(temb_rows=1))
        add("odd T", T + 1 if T % 2 else T - 1, cfg_seqs(1, L), sampler(1, T, L))   # (the same rows: S = (T + 1) / 2)
        add("zero row in place", T, cfg_seqs(1, L), sampler(1, T, L, zr_M=2 * ((T + 1) // 2)))
        add("graph mode, zero row in place", T, cfg_seqs(1, L), sampler(1, T, L, graph_mode=1, zr_M=2 * ((T + 1) // 2)))
        add("layers 0 and 1 tapped", T, cfg_seqs(1, L), sampler(1, T, L, tap_mask=3))
        add("dedup off", T, cfg_seqs(1, L), sampler(1, T, L, dedup_on=0))
        nl = config(name).num_hidden_layers
        heads = [0] * nl
        heads[0], heads[nl // 2] = 1, 2
        add("maps stopping at a middle layer", T, [(0, L, 0), (0, L, 0)], dict(map_last=nl // 2, map_heads=heads))
    names = [r[0] for r in rows]
    assert len(set(names)) == len(names)
    return rows


REFUSALS = [("forward: condition slot not set", [(0, 5, 0), (1, 0, 0)]), ("forward: condition slot not set", [(40, 5, 0)]),
            ("forward: condition slot not set", [(-1, 5, 0)]),
            ("forward: the condition slots that run cross-attention in one call must share L", [(0, 5, 0), (1, 6, 0)])]


def compact(step):
    return {k: v for k, v in step.items() if v != STEP_DEFAULTS.get(k, 0)}


def plan(cfg_name, T, seqs, fields):
    from ace355 import native
    return native.dit_pass_plan(config(cfg_name), T, seqs, **fields)


def row_of(name, cfg_name, T, seqs, fields):
    p = plan(cfg_name, T, seqs, fields)
    steps = [compact(s) for s in p.pop("steps")]
    p["sha256"] = hashlib.sha256(json.dumps(steps, sort_keys=True).encode()).hexdigest()
    p["kinds"] = {}
    for s in steps:
        k = s["kind"] + (":" + s["path"] if s["kind"] == "gemm" else "")
        p["kinds"][k] = p["kinds"].get(k, 0) + 1
    if name in STEPS_KEPT:
        p["steps"] = [s for s in steps if STEPS_KEPT[name] is None or s.get("layer", -1) in STEPS_KEPT[name]]
    return p


def evaluate():
    return [{"name": n, "config": c, "T": T, "seqs": [list(s) for s in seqs], "fields": f, "plan": row_of(n, c, T, seqs, f)} for n, c, T, seqs, f in table_requests()]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import ace355  # noqa: F401
    if "--write" in sys.argv:
        with open(TABLE, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(row) for row in evaluate()) + "\n]\n")
        print("wrote", TABLE)
    elif "--plans" in sys.argv:
        print(json.dumps(evaluate()))
