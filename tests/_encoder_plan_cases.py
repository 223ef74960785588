"""The encoder pass requests whose plans tests/encoder_plan_table.json records, and the evaluator behind tests/test_encoder_plan_cpu.py.

    python tests/_encoder_plan_cases.py --write     regenerate the table (after a deliberate change of csrc/encoder_plan.h)

A request is (configuration name, N, S, fields): the arguments of native.encoder_pass_plan.  No GPU is needed: ace355_encoder_pass_plan
evaluates the library's pure plan_encoder_pass.  The table keeps a plan's facts, its launcher calls per kind and a SHA-256 over all its
steps; the rows on the small configurations also keep the steps of layer 0 and the final norm, so that a change shows which calls moved.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "encoder_plan_table.json")

# (hidden, intermediate, heads, kv heads, layers): the full-size text encoder / 0.6B LM, 1.7B LM, lyric and timbre encoder, detokenizer
# (config.py), and the small configurations of the GPU tests (test_encoder_lifecycle_gpu.py TINY; _lm_oracle.py tiny / wide)
CONFIGS = {"textenc": (1024, 3072, 16, 8, 28), "lm17": (2048, 6144, 16, 8, 28), "lyric": (2048, 6144, 16, 8, 8), "timbre": (2048, 6144, 16, 8, 4),
           "detok": (2048, 6144, 16, 8, 2), "tiny": (256, 768, 2, 1, 2), "tiny65": (256, 768, 2, 1, 65), "wide": (512, 1024, 16, 8, 2)}


def cache(pos0, max_pos, max_seqs, first=1):
    return dict(causal=1, has_cache=1, pos0=pos0, max_pos=max_pos, max_seqs=max_seqs, has_first=first)


def table_requests():
    rows = []
    add = lambda what, cfg, N, S, **fields: rows.append((f"{cfg}: {what}", cfg, N, S, fields))
    # full size
    add("caption batch 16 x 256", "textenc", 16, 256, causal=1)
    add("lyric batch 8 x 2048", "textenc", 8, 2048, causal=1)
    for cfg in ("textenc", "lm17"):
        add("LM prefill, CFG pair x 8 songs, 300 columns, left padding", cfg, 16, 300, **cache(0, 4096, 16))
        for length in (256, 257, 1024, 1025, 4096):
            add(f"LM decode step at length {length}, left padding", cfg, 16, 1, **cache(length - 1, 4096, 16))
    add("lyrics 2 x 512 with key counts, layers alternate sliding / full", "lyric", 2, 512, has_kv_len=1, sliding_window=128, sliding_layer_mask=0x55)
    add("4 reference clips x 750", "timbre", 4, 750, sliding_window=128, sliding_layer_mask=0x5)
    add("detokenizer, 750 windows of 5", "detok", 750, 5, sliding_window=128, sliding_layer_mask=0x1)
    add("tokenizer, 750 windows of 1 + 5", "detok", 750, 6, sliding_window=128, sliding_layer_mask=0x1)
    # the small configurations of the GPU tests, on each path
    add("lyrics 2 x 70 with key counts, layer 0 sliding", "tiny", 2, 70, has_kv_len=1, sliding_window=16, sliding_layer_mask=0x1)
    add("3 reference clips x 33, layer 0 sliding", "tiny", 3, 33, sliding_window=16, sliding_layer_mask=0x1)
    add("detokenizer, 14 windows of 5", "tiny", 14, 5, sliding_window=128, sliding_layer_mask=0x1)
    add("tokenizer, 14 windows of 6", "tiny", 14, 6, sliding_window=128, sliding_layer_mask=0x1)
    for S in (1, 64, 65, 130):
        add(f"text 2 x {S}", "tiny", 2, S, causal=1)
    add("text 1 x 8, more layers than mask bits", "tiny65", 1, 8, causal=1, sliding_window=16, sliding_layer_mask=(1 << 64) - 1)
    for cfg in ("tiny", "wide"):
        for P in (1, 17, 64, 65, 130):
            add(f"LM prefill 3 x {P}, left padding", cfg, 3, P, **cache(0, 1100, 4))
        for length in (61, 256, 257, 1024, 1025, 1100):
            add(f"LM decode step at length {length}, left padding", cfg, 3, 1, **cache(length - 1, 1100, 4))
    add("LM prefill that fills the cache", "tiny", 2, 8, **cache(0, 8, 2))
    add("LM prefill without first keys", "tiny", 2, 8, **cache(0, 8, 2, first=0))
    names = [r[0] for r in rows]
    assert len(set(names)) == len(names)
    return rows


TINY = dict(zip(("hidden_size", "intermediate_size", "num_heads", "num_kv_heads", "num_layers"), CONFIGS["tiny"]))
REFUSALS = [("encoder_layers: KV cache position", dict(N=2, S=1, **cache(8, 8, 2))),
            ("encoder_layers: KV cache position", dict(N=2, S=2, **cache(3, 8, 2))),
            ("encoder_layers: KV cache position", dict(N=2, S=9, **cache(0, 8, 2))),
            ("encoder_layers: KV cache position", dict(N=2, S=1, **{**cache(0, 8, 2), "causal": 0})),
            ("kv store: cache bounds", dict(N=3, S=4, **cache(0, 8, 2))),
            ("decode attention: cache bounds", dict(N=2, S=1, **cache(3, 8, 2, first=0))),
            ("causal attention: sizes", dict(N=65536, S=1, causal=1)),
            ("gemm: K must be a multiple of 64", dict(N=1, S=4, intermediate_size=800)),
            ("gemm: A and W must each be smaller than 4 GB (32-bit DMA offsets)", dict(N=1 << 11, S=1 << 12)),
            ("attention: Hq % Hkv", dict(N=1, S=4, num_heads=3, num_kv_heads=2))]


def plan(cfg_name, N, S, fields):
    from ace355 import native
    return native.encoder_pass_plan(*CONFIGS[cfg_name], N, S, **fields)


def row_of(cfg_name, N, S, fields):
    p = plan(cfg_name, N, S, fields)
    steps = p.pop("steps")
    p["sha256"] = hashlib.sha256(json.dumps(steps, sort_keys=True).encode()).hexdigest()
    if cfg_name in ("tiny", "wide"):
        p["steps"] = [s for s in steps if s["layer"] <= 0]
    return p


def evaluate():
    return [{"name": n, "config": c, "N": N, "S": S, "fields": f, "plan": row_of(c, N, S, f)} for n, c, N, S, f in table_requests()]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import ace355  # noqa: F401
    if "--write" in sys.argv:
        with open(TABLE, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(row) for row in evaluate()) + "\n]\n")
        print("wrote", TABLE)
