"""The attention requests whose launch plans tests/attn_plan_table.json records, and the evaluator behind tests/test_attn_plan_cpu.py.

    python tests/_attn_plan_cases.py --write            regenerate the table (after a deliberate change of the heuristics in csrc/attn_plan.h)
    python tests/_attn_plan_cases.py --plans [--krot n]   print the table requests' plans of THIS process (its ACE355_ATTN_* environment) as JSON

A request is a dict of ace355_attn_request fields (include/ace355.h); fields left out are 0 (no scratch, no mask, the whole chip).  No GPU
is needed: ace355_attn_plan evaluates the library's pure plan_attention.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "attn_plan_table.json")
PART = 16 << 20   # floats of split-KV scratch the unit hooks (csrc/api.hip) and the DiT handle (csrc/dit.hip) lend

# tests/test_kernels_gpu.py::test_attention's rows, (N, Sq, Skv, Hq, Hkv, window), each with the launch it was chosen for:
# (kernel, its template argument, kv_split).  The GPU test imports this list and asserts the form before it launches.
ATTENTION_ROWS = [
    # small problems and group sizes other than Hq = 2 Hkv stay on attn3_kernel<4> (128-query blocks): the one-song CFG self-attention, full
    # and banded, ragged last blocks and key tiles, a single key
    ((2, 375, 375, 16, 8, -1), ("attn3", 4, 1)), ((2, 375, 375, 16, 8, 128), ("attn3", 4, 1)), ((1, 300, 300, 2, 1, 16), ("attn3", 4, 1)),
    ((2, 375, 769, 16, 8, -1), ("attn3", 4, 2)),   # 96 workgroups x 13 key tiles: split-KV in 2 parts
    ((1, 20, 33, 2, 1, -1), ("attn3", 4, 1)), ((1, 1500, 1500, 4, 2, 128), ("attn3", 4, 1)), ((1, 129, 129, 2, 2, 128), ("attn3", 4, 1)),
    ((1, 64, 1, 2, 1, -1), ("attn3", 4, 1)),
    # Hq = 2 Hkv takes attn_gqa_kernel<NWH> once its grid fills the chip: NWH = 6 (12 waves, 192-row blocks: configs[2]'s self-attention,
    # full and banded, with a ragged last block 1500 = 7 x 192 + 156, and its cross-attention shape; the metric's launches at N = 16,
    # 375 = 192 + 183)
    ((6, 1500, 1500, 16, 8, -1), ("gqa", 6, 1)), ((6, 1500, 1500, 16, 8, 128), ("gqa", 6, 1)), ((6, 1500, 769, 16, 8, -1), ("gqa", 6, 1)),
    ((16, 375, 375, 16, 8, -1), ("gqa", 6, 1)), ((16, 375, 375, 16, 8, 128), ("gqa", 6, 1)),
    # the metric's cross-attention at Nc = 8: 96-row blocks, where the 12-wave key-split attn_rot_kernel<3> replaces attn_gqa_kernel<3>
    ((8, 375, 769, 16, 8, -1), ("rot", 3, 1)),
    ((16, 375, 769, 16, 8, -1), ("gqa", 6, 1)),
    ((12, 375, 375, 16, 8, 128), ("gqa", 4, 1)),   # 8 waves, 128-row blocks
    # other group sizes stay on attn3_kernel: <8> (256-query blocks; Sq >= 1024 and heads x ceil(Sq / 256) >= 512) and <4>
    ((6, 1500, 1500, 16, 16, -1), ("attn3", 8, 1)), ((6, 1500, 1500, 16, 16, 128), ("attn3", 8, 1)), ((4, 375, 375, 8, 8, 128), ("attn3", 4, 1)),
    # batch-1 requests: few workgroups with long key walks (>= 8 tiles) take the split-KV path of attn3_kernel<4> + attn_merge_kernel: the
    # cross-attention of one conditional sequence (48 workgroups x 13 tiles -> 4 parts), configs[0]'s shapes (Sq = 125: 16 workgroups ->
    # 4 parts; banded self-attention, not split), a ragged split (9 tiles in 4 parts)
    ((1, 375, 769, 16, 8, -1), ("attn3", 4, 4)), ((1, 125, 769, 16, 8, -1), ("attn3", 4, 4)), ((2, 125, 125, 16, 8, 16), ("attn3", 4, 1)),
    ((1, 200, 550, 4, 2, -1), ("attn3", 4, 4)),
    # the smallest shapes that reach what nothing above does: attn_rot_kernel<3> with a ragged 96-row block (100 = 96 + 4) and a ragged key
    # tile (130 = 2 x 64 + 2) - under K rotation mode 0 the same shape is ONE_ORDER_ROW below - and an 8-part split (16 tiles, 16 workgroups)
    ((16, 100, 130, 16, 8, -1), ("rot", 3, 1)), ((1, 125, 1000, 16, 8, -1), ("attn3", 4, 8)),
]
# test_attention_one_order: the row that takes attn_gqa_kernel<3> once ace355_gemm_set_k_rotation(0) keeps the key-split kernel off
ONE_ORDER_ROW = ((16, 100, 130, 16, 8, -1), ("gqa", 3, 1))
# every (kernel, template argument) plan_attention can emit, and the split counts of its heuristic
ALL_FORMS = {("attn3", 4), ("attn3", 8), ("gqa", 3), ("gqa", 4), ("gqa", 6), ("rot", 3)}
ALL_SPLITS = {1, 2, 4, 8}

# tests/test_cond_gpu.py::test_attention_key_padding_mask's shapes (ace355_attention_masked)
MASKED_ROWS = [(3, 300, 300, 2, 1, 128), (2, 200, 200, 4, 2, 16), (2, 129, 129, 2, 2, -1)]

# tests/test_attention_keys_gpu.py's rows (the softmax weights read back one by one through a one-hot V, tests/_attn_keys.py): small
# shapes, each with the launch it was chosen for and, where it needs them, options: "krot" = the K rotation mode the case runs under
# (ace355_gemm_set_k_rotation), "lens" = the key-padding mask's lengths (ace355_attention_masked), "pairs" = the (n, h) the fp64 reference
# is computed for (all of them when left out).
def _lens(N, cycle):
    return tuple(cycle[i % len(cycle)] for i in range(N))


KEY_ROWS = [
    # attn3_kernel<4>: ragged block and tile, a narrow band, the product's window with a group size of 3, a single key
    ((1, 70, 70, 2, 1, -1), ("attn3", 4, 1), {}), ((1, 200, 200, 2, 1, 16), ("attn3", 4, 1), {}), ((1, 300, 300, 3, 1, 128), ("attn3", 4, 1), {}),
    ((1, 64, 1, 2, 1, -1), ("attn3", 4, 1), {}),
    # attn3_kernel<8>: 1030 = 4 x 256 + 6, a ragged fifth block of 6 rows; the banded row's reference covers 8 (n, h) with both end
    # sequences and the first and last head, at full Sq x Skv (every other head is still held to the zeros outside the band)
    ((4, 1030, 130, 32, 32, -1), ("attn3", 8, 1), {}),
    ((4, 1030, 1030, 32, 32, 40), ("attn3", 8, 1), {"pairs": ((0, 0), (0, 31), (3, 0), (3, 31), (1, 7), (2, 13), (1, 20), (2, 26))}),
    # attn_gqa_kernel<6>; Hkv = 16: two KV heads per XCD slot (hg = 2); Hkv = 3: the generic workgroup order, a grid of 232 for 225 units
    ((28, 100, 130, 16, 8, -1), ("gqa", 6, 1), {}), ((28, 200, 200, 16, 8, 16), ("gqa", 6, 1), {}), ((14, 100, 130, 32, 16, -1), ("gqa", 6, 1), {}),
    ((75, 100, 130, 6, 3, -1), ("gqa", 6, 1), {}),
    # attn_gqa_kernel<4>
    ((14, 150, 130, 16, 8, -1), ("gqa", 4, 1), {}), ((14, 150, 150, 16, 8, 16), ("gqa", 4, 1), {}), ((38, 150, 150, 6, 3, 16), ("gqa", 4, 1), {}),
    # attn_rot_kernel<3>
    ((8, 100, 130, 16, 8, -1), ("rot", 3, 1), {}), ((8, 100, 100, 16, 8, 16), ("rot", 3, 1), {}), ((22, 100, 130, 6, 3, -1), ("rot", 3, 1), {}),
    ((4, 100, 130, 32, 16, -1), ("rot", 3, 1), {}),
    # attn_gqa_kernel<3>: K rotation mode 0 keeps the key-split kernel off
    ((8, 100, 130, 16, 8, -1), ("gqa", 3, 1), {"krot": 0}), ((8, 100, 100, 16, 8, 16), ("gqa", 3, 1), {"krot": 0}),
    # split-KV on attn3_kernel<4>: 4 parts; 9 tiles in 4 parts of 3 (part 3 empty); 8 parts; banded in 4 parts (the edge blocks walk 6 and 7
    # tiles in parts of 2: part 3 empty); 2 parts (72 workgroups x 9 tiles, group size 3, three sequences)
    ((1, 100, 520, 8, 4, -1), ("attn3", 4, 4), {}), ((1, 200, 550, 4, 2, -1), ("attn3", 4, 4), {}), ((1, 100, 1030, 16, 8, -1), ("attn3", 4, 8), {}),
    ((1, 700, 700, 2, 1, 200), ("attn3", 4, 4), {}), ((3, 100, 520, 24, 8, -1), ("attn3", 4, 2), {}),
    # key-padding masks on every kernel: each row's lengths hold Skv, 0, values that are no multiple of 64 and, on the banded rows, one
    # short enough that the later queries of a live sequence see no key at all (the uniform rule beside ordinary rows)
    ((3, 300, 300, 2, 1, 128), ("attn3", 4, 1), {"lens": (300, 100, 0)}),
    ((28, 100, 100, 16, 8, -1), ("gqa", 6, 1), {"lens": _lens(28, (100, 0, 37, 64, 99, 1, 65))}),
    ((14, 150, 150, 16, 8, 16), ("gqa", 4, 1), {"lens": _lens(14, (150, 0, 37, 100, 128, 1, 149))}),
    ((8, 100, 100, 16, 8, 16), ("rot", 3, 1), {"lens": (100, 0, 37, 64, 70, 1, 99, 50)}),
    ((8, 100, 100, 16, 8, 16), ("gqa", 3, 1), {"lens": (100, 0, 37, 64, 70, 1, 99, 50), "krot": 0}),
]


def key_row_id(row):
    shape, (kernel, nw, kv_split), opts = row
    return "-".join(["x".join(str(d) for d in shape), f"{kernel}{nw}" + (f"split{kv_split}" if kv_split > 1 else "")]
                    + (["masked"] if "lens" in opts else []) + ([f"krot{opts['krot']}"] if "krot" in opts else []))


def key_row_plan(row):
    """The row's plan as the GPU test asks for it: under the scratch the unit hooks lend and, for the moment, the row's K rotation mode."""
    from ace355 import native
    shape, _form, opts = row
    prev = native.gemm_set_k_rotation(opts["krot"]) if "krot" in opts else None
    try:
        return native.attn_plan(*shape, part_floats=native.ATTN_HOOK_PART_FLOATS, **({"has_kv_len": 1} if "lens" in opts else {}))
    finally:
        if prev is not None:
            native.gemm_set_k_rotation(prev)


HQ, HKV, WINDOW, L_COND = 16, 8, 128, 769   # the DiT at full size; 769 condition tokens as in the GPU tests' cross-attention shapes


def request(shape, **fields):
    return {**dict(zip(("N", "Sq", "Skv", "Hq", "Hkv", "window"), shape)), **fields}


def dit_launches(songs, T, cu_slots=0):
    """The attention launches of a sampler step of the full-size DiT for `songs` songs with CFG at T latent frames, read from the library's
    pass plan (native.dit_pass_plan): self-attention over both halves (layer 0 projects the conditional half only), full and banded, and
    cross-attention over the conditional half."""
    import ace355
    from ace355 import native
    cfg = ace355.DitConfig()
    plan = native.dit_pass_plan(cfg, T, [(0, L_COND, 0)] * songs + [(1, L_COND, 1)] * songs, temb_rows=1, dup_half=1, cu_slots=cu_slots,
                                prefetch=int(not cu_slots))
    attn = [st for st in plan["steps"] if st["kind"] in ("attn_self", "attn_cross")]
    first = lambda cond: next(st for st in attn if cond(st))
    rq = lambda st: request((st["seqs"], st["Sq"], st["Skv"], cfg.num_attention_heads, cfg.num_key_value_heads, st["window"]), part_floats=PART, cu_slots=cu_slots)
    layer0 = first(lambda st: st["kind"] == "attn_self" and st["layer"] == 0)
    assert layer0["window"] == WINDOW and all(st["mx_out"] == 0 for st in attn)
    return [("self, full", rq(first(lambda st: st["kind"] == "attn_self" and st["layer"] > 0 and st["window"] < 0))),
            ("self, sliding", rq(first(lambda st: st["kind"] == "attn_self" and st["layer"] > 0 and st["window"] >= 0))),
            ("self, layer 0 (sliding), conditional half", rq(layer0)), ("cross", rq(first(lambda st: st["kind"] == "attn_cross")))]


def table_requests():
    rows = []
    add = lambda group, items: rows.extend((f"{group}: {n}", r) for n, r in items)
    add("test_attention", [(str(s), request(s, part_floats=PART)) for s, _form in ATTENTION_ROWS])
    add("test_attention_key_padding_mask", [(str(s), request(s, part_floats=PART, has_kv_len=1)) for s in MASKED_ROWS])
    # (the table holds this process's plans: a row that runs under another K rotation mode is its default-mode twin here)
    add("test_attention_keys", [(str(s) + (" masked" if "lens" in o else ""), request(s, part_floats=PART, **({"has_kv_len": 1} if "lens" in o else {})))
                                for s, _form, o in KEY_ROWS if "krot" not in o])
    for songs in (1, 2, 4, 8):   # (by default a 2-song request runs as two chains of one song: the first group's launches)
        add(f"{songs} song{'s' if songs > 1 else ''}, CFG, T = 750", dit_launches(songs, 750))
    add("dual-chain sampler, 4 songs per chain, 128 CUs, T = 750", dit_launches(4, 750, cu_slots=128))
    add("1 song, CFG, T = 3000", dit_launches(1, 3000))
    add("1 song, CFG, T = 6000", dit_launches(1, 6000))
    add("8 songs, CFG, T = 3000", dit_launches(8, 3000))
    add("MXFP8 output", [("self, full, metric batch", request((16, 375, 375, HQ, HKV, -1), part_floats=PART, mx_out=1)),
                         ("cross, metric batch (96-row blocks stay on the GQA kernel)", request((8, 375, L_COND, HQ, HKV, -1), part_floats=PART, mx_out=1))])
    # encoder.hip's stacks lend no scratch; the condition encoders carry a key-padding mask (sizes of the gemm plan table's encoder rows)
    add("encoders", [("lyric 2 x 200", request((2, 200, 200, HQ, HKV, WINDOW), has_kv_len=1)), ("timbre 3 x 96", request((3, 96, 96, HQ, HKV, -1), has_kv_len=1)),
                     ("detokenizer 50 x 5", request((50, 5, 5, HQ, HKV, -1))), ("audio tokenizer 100 x 6", request((100, 6, 6, HQ, HKV, -1)))])
    add("edge", [("split refused: the scratch is too small for any part count", request((1, 375, 769, HQ, HKV, -1), part_floats=1 << 20)),
                 ("one pass by the heuristic (4 parts do not fit 2 Mi floats), 2 parts when ACE355_ATTN_KVSPLIT forces them", request((1, 375, 769, HQ, HKV, -1), part_floats=2 << 20)),
                 ("no scratch", request((1, 375, 769, HQ, HKV, -1)))])
    names = [n for n, _r in rows]
    assert len(set(names)) == len(names)
    return rows


def plan(rq):
    from ace355 import native
    return native.attn_plan(**rq)


def evaluate(krot=None):
    from ace355 import native
    if krot is not None:
        native.gemm_set_k_rotation(krot)
    return [{"name": n, "request": r, "plan": plan(r)} for n, r in table_requests()]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import ace355  # noqa: F401
    if "--write" in sys.argv:
        with open(TABLE, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(row) for row in evaluate()) + "\n]\n")
        print("wrote", TABLE)
    elif "--plans" in sys.argv:
        print(json.dumps(evaluate(int(sys.argv[sys.argv.index("--krot") + 1]) if "--krot" in sys.argv else None)))
