"""The GEMM requests whose launch plans tests/gemm_plan_table.json records, and the evaluator behind tests/test_gemm_plan_cpu.py.

    python tests/_gemm_plan_cases.py --write          regenerate the table (after a deliberate change of the heuristics in csrc/gemm.hip)
    python tests/_gemm_plan_cases.py --plans [--krot n]   print the table requests' plans of THIS process (its ACE355_GEMM_* environment) as JSON

A request is a dict of ace355_gemm_request fields (include/ace355.h); fields left out are 0, `aligned` is 1.  Modes: 0 store bf16, 1 store
f32, 2 residual, 3 SwiGLU, 4 head-norm + RoPE.  No GPU is needed: ace355_gemm_plan evaluates the library's pure plan_gemm.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "gemm_plan_table.json")
VERIFIED, REFUSED = 1, 0

# The DiT pass rows are read from the library's pass plan (native.dit_pass_plan) at full size, T = 750, 769 condition tokens
S_FULL, L_COND = 375, 769

# test_gemm_launches_are_bit_reproducible's rows with the regime each was written for: (MT, WNW, NTW, PERS, NS, split-K).  The GPU test
# imports this list, so the shapes exist once.
BIT_REPRODUCIBLE = [
    # the 4-wave two-stage kernels with two workgroups per CU (more tiles than CUs, too few for the 8-wave forms): the regime whose launches were not
    # reproducible until round 6 (MFMA destination overlapping srcB; consecutive MFMAs sharing srcA beside a co-resident bf16 epilogue)
    ("swiglu", 400, 12288, 2048, 16, (2, 2, 2, 0, 2, False)), ("swiglu", 288, 12288, 2048, 16, (2, 2, 2, 0, 2, False)),
    ("store_bf16", 520, 8192, 2048, 16, (2, 2, 2, 0, 2, False)), ("headnorm", 520, 8192, 2048, 16, (2, 2, 2, 0, 2, False)),
    ("store_f32", 520, 8192, 2048, 8, (2, 2, 2, 0, 2, False)), ("residual", 520, 8192, 2048, 8, (2, 2, 2, 0, 2, False)),
    # deep-pipeline 4-wave kernels (one workgroup per CU), 64-row tiles, ordered split-K
    ("swiglu", 48, 12288, 2048, 8, (2, 2, 2, 0, 4, False)), ("headnorm", 400, 4096, 2048, 8, (1, 2, 2, 0, 4, False)),
    ("residual", 400, 2048, 6144, 8, (1, 2, 2, 0, 4, True)), ("residual", 375, 2048, 2048, 8, (1, 2, 2, 0, 4, True)),
    # the 8-wave pair loops at the metric batch (persistent 192x256, one-round 192x256, 192x128)
    ("swiglu", 6000, 12288, 2048, 4, (3, 4, 2, 1, 2, False)), ("headnorm", 6000, 4096, 2048, 4, (3, 4, 2, 1, 2, False)),
    ("residual", 6000, 2048, 6144, 4, (3, 4, 2, 0, 2, False)), ("store_bf16", 400, 12288, 2048, 8, (3, 4, 1, 0, 3, False)),
]
# test_gemm_tile_forms_give_the_same_bits: fp32 store with K rotation off, ACE355_GEMM_BIG -> the regime (as above) of each shape's launch.
# 4-wave: 6000 rows take two rounds of 192-row tiles (two stages), 1536 rows one round of 128-row tiles (deep); the forced 8-wave tiles stay
# one round (no persistent form) and the 192x128 one has its three stages.
TILE_FORMS = [(6000, 2048, 2048), (1536, 2048, 6144)]
TILE_FORM_OF_BIG = {"0": [(3, 2, 2, 0, 2, False), (2, 2, 2, 0, 4, False)], "2": [(3, 4, 2, 0, 2, False)] * 2, "3": [(3, 4, 1, 0, 3, False)] * 2}


def entry_request(kind, M, N, K):
    """What the unit entry points (ace355_gemm_bf16 / _fused / _residual / _headnorm, csrc/api.hip) send for a test's `kind`."""
    mode = {"store_bf16": 0, "store_f32": 1, "residual": 2, "swiglu": 3, "headnorm": 4}[kind]
    rq = dict(M=M, N=N, K=K, mode=mode, counters=int(kind != "swiglu"))
    if kind == "headnorm":
        rq.update(hn_q_cols=N // 2, hn_qk_cols=N // 4 * 3)
    return rq


# The GEMMs of a pass the table names, as (projection, layer; -1: the last layer), and the request fields it records for each besides M, N, K,
# mode, counters and cu_slots.  A field it does not record is 0 in that launch's request (asserted).
PASS_ROWS = [("patchify", ("patchify", None), ()),
             ("qkv layer 0", ("qkv", 0), ("fp8", "hn_q_cols", "hn_qk_cols", "vt_offered", "vt_heads", "fold_consumer", "pf_x")),
             ("qkv", ("qkv", 1), ("fp8", "hn_q_cols", "hn_qk_cols", "vt_offered", "vt_heads", "fold_consumer", "pf_x")),
             ("o_proj", ("o", 1), ("fp8", "fold_producer", "pf_x")),
             ("cross q", ("cross_q", 1), ("hn_q_cols", "hn_qk_cols", "fold_consumer", "pf_x")),
             ("cross o_proj", ("cross_o", 1), ("fold_producer", "pf_x")),
             ("gate|up", ("gate_up", 1), ("fp8", "fold_consumer", "pf_x")),
             ("down", ("down", 1), ("fp8", "fold_producer", "pf_x")),
             ("down last layer", ("down", -1), ("fp8", "pf_x")),
             ("proj_out", ("out", None), ())]


def step_request(st, kv_heads, cu_slots):
    """The ace355_gemm_request of a pass plan's GEMM step.  pf_x: the prefetch workgroups gemm_prefetch_plan attaches for the step's target,
    which ace355_gemm_plan reports for that target's own request.  counters: the handle lends its turn counters to every launch of the pass
    (the MXFP8 launcher takes none; plan_gemm does not read the field for fp8)."""
    from ace355 import native
    pf_x = 0
    if st["next_proj"] is not None:
        pf_x = native.gemm_plan(st["next_M"], st["next_N"], st["next_K"], st["next_mode"], cu_slots=cu_slots)["next_pf_x"]
    return dict(M=st["M"], N=st["N"], K=st["K"], mode=st["mode"], fp8=int(st["path"] != "bf16"), hn_q_cols=st["hn_q_cols"], hn_qk_cols=st["hn_qk_cols"],
                vt_offered=st["vt_offered"], vt_heads=kv_heads if st["vt_offered"] else 0, fold_producer=int(st["nf_split"] >= 0),
                fold_consumer=int(st["nc_rowsq"] >= 0), pf_x=pf_x, counters=1, cu_slots=cu_slots)


def forward_core(M, Mc, fold, fp8=False, cu_slots=0):
    """The GEMMs of a sampler step of the full-size DiT for M rows of which Mc are conditional (cross-attention) rows, the others the CFG
    null branch, read from the library's pass plan: (name, request).  fold False: the same step with ACE355_NORM_FOLD=0."""
    import ace355
    from ace355 import native
    cfg = ace355.DitConfig()
    N, Nc = M // S_FULL, Mc // S_FULL
    plan = native.dit_pass_plan(cfg, 2 * S_FULL, [(0, L_COND, 0)] * Nc + [(1, L_COND, 1)] * (N - Nc), temb_rows=1, dup_half=int(N > Nc),
                                nf_on=int(fold), nf_emb_on=1, nf_rows=27, nf_cap_M=M, precision=int(fp8), cu_slots=cu_slots, prefetch=int(not cu_slots))
    gemms = {(st["proj"], st["layer"] if st["layer"] >= 0 else None): st for st in plan["steps"] if st["kind"] == "gemm"}
    out = []
    for name, (proj, layer), recorded in PASS_ROWS:
        rq = step_request(gemms[(proj, cfg.num_hidden_layers - 1 if layer == -1 else layer)], cfg.num_key_value_heads, cu_slots)
        keep = ("M", "N", "K", "mode") + recorded + ("counters", "cu_slots")
        assert all(v == 0 for k, v in rq.items() if k not in keep), (name, rq)
        out.append((name, {k: v for k, v in rq.items() if k in keep}))
    return out


def encoder_stack(M, d, qd, kvd, f):
    """The four projections of a layer of encoder.hip encoder_layers."""
    return [("qkv", dict(M=M, N=qd + 2 * kvd, K=d, mode=4, hn_q_cols=qd, hn_qk_cols=qd + kvd)), ("o_proj", dict(M=M, N=d, K=qd, mode=2, counters=1)),
            ("gate|up", dict(M=M, N=2 * f, K=d, mode=3)), ("down", dict(M=M, N=d, K=f, mode=2, counters=1))]


def table_requests():
    rows = []
    add = lambda group, items: rows.extend((f"{group}: {n}", r) for n, r in items)
    add("one song, CFG, sampler (folded norms)", forward_core(750, 375, True))
    add("one song, CFG, plain forward", forward_core(750, 375, False))   # (group names as recorded; see forward_core for fold False)
    add("one song, no CFG", forward_core(375, 375, False))
    add("metric batch, sampler", forward_core(6000, 3000, True))
    add("metric batch, plain forward", forward_core(6000, 3000, False))
    add("metric batch, MXFP8", forward_core(6000, 3000, False, fp8=True))
    add("dual-chain sampler, 4 songs per chain, 128 CUs", forward_core(3000, 1500, True, cu_slots=128))
    # the four encoder handles at the sizes of their full-size tests (test_cond_gpu, test_lmhints_gpu, test_textenc_gpu)
    add("lyric encoder 2 x 200", encoder_stack(400, 2048, 2048, 1024, 6144))
    add("timbre encoder 3 x 96", encoder_stack(288, 2048, 2048, 1024, 6144))
    add("detokenizer 50 x 5", encoder_stack(250, 2048, 2048, 1024, 6144))
    add("audio tokenizer 100 x 6", encoder_stack(600, 2048, 2048, 1024, 6144))
    add("text encoder 3 x 256", encoder_stack(768, 1024, 2048, 1024, 3072))
    add("bit-reproducible", [(f"{k} {M}x{N}x{K}", entry_request(k, M, N, K)) for k, M, N, K, _reps, _regime in BIT_REPRODUCIBLE])
    add("tile forms", [(f"store_f32 {M}x{N}x{K}", entry_request("store_f32", M, N, K)) for M, N, K in TILE_FORMS])
    add("edge", [("ragged N (not a multiple of the tile)", dict(M=520, N=2000, K=2048, mode=0)),
                 ("misaligned output (scalar epilogue)", dict(M=400, N=4096, K=2048, mode=0, aligned=0)),
                 ("misaligned head epilogue (falls back to two kernels)", dict(M=400, N=4096, K=2048, mode=4, aligned=0, hn_q_cols=2048, hn_qk_cols=3072)),
                 ("head epilogue on the 192x128 tile", dict(M=750, N=8192, K=2048, mode=4, hn_q_cols=4096, hn_qk_cols=6144)),
                 ("residual without counters (atomic split-K)", dict(M=375, N=2048, K=2048, mode=2)),
                 ("fold producer without counters (no split)", dict(M=375, N=2048, K=2048, mode=2, fold_producer=1))])
    names = [n for n, _r in rows]
    assert len(set(names)) == len(names)
    return rows


def plan(request, placement=VERIFIED):
    from ace355 import native
    return native.gemm_plan(**{"aligned": 1, **request, "placement": placement})


def evaluate(krot=None):
    from ace355 import native
    if krot is not None:
        native.gemm_set_k_rotation(krot)
    return [{"name": n, "request": r, "verified": plan(r, VERIFIED), "refused": plan(r, REFUSED)} for n, r in table_requests()]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import ace355  # noqa: F401
    if "--write" in sys.argv:
        with open(TABLE, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(row) for row in evaluate()) + "\n]\n")
        print("wrote", TABLE)
    elif "--plans" in sys.argv:
        print(json.dumps(evaluate(int(sys.argv[sys.argv.index("--krot") + 1]) if "--krot" in sys.argv else None)))
