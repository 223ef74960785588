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

# The DiT at full size (config.DitConfig defaults) and the prefetch rule of dit.hip / gemm_prefetch_plan: a launch carries prefetch
# workgroups for the NEXT projection when that one has at most 800 rows and a residual or head epilogue.
D, QD, KVD, F, IN2, OUT2 = 2048, 2048, 1024, 6144, 384, 128
QKV = QD + 2 * KVD
PF_X, PF_MAX_ROWS = 24, 800

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


def _pf(next_rows, next_mode):
    return PF_X if 0 < next_rows <= PF_MAX_ROWS and next_mode in (2, 4) else 0


def forward_core(M, Mc, fold, fp8=False, cu_slots=0, prefetch=True):
    """Every GEMM of dit.hip forward_core for M rows of which Mc are conditional (cross-attention) rows: (name, request)."""
    c = dict(counters=1, cu_slots=cu_slots)
    pf = (lambda rows, mode: _pf(rows, mode)) if prefetch and not fp8 else (lambda rows, mode: 0)
    out = [("patchify", dict(M=M, N=D, K=IN2, mode=1, **c))]
    for layer0 in (True, False):
        # layer 0 of a CFG forward projects q / k / v for the conditional half only (dedup0), and its input norm is never folded
        Mq = Mc if layer0 and not fp8 and M == 2 * Mc else M
        out.append((f"qkv{' layer 0' if layer0 else ''}", dict(M=Mq, N=QKV, K=D, mode=4, fp8=int(fp8), hn_q_cols=QD, hn_qk_cols=QD + KVD, vt_offered=1,
                                                                vt_heads=KVD // 128, fold_consumer=int(fold and not layer0), pf_x=pf(M, 2), **c)))
    out.append(("o_proj", dict(M=M, N=D, K=QD, mode=2, fp8=int(fp8), fold_producer=int(fold), pf_x=pf(Mc, 4), **c)))
    out.append(("cross q", dict(M=Mc, N=QD, K=D, mode=4, hn_q_cols=QD, hn_qk_cols=QD, fold_consumer=int(fold), pf_x=pf(Mc, 2), **c)))
    out.append(("cross o_proj", dict(M=Mc, N=D, K=QD, mode=2, fold_producer=int(fold), pf_x=pf(M, 3), **c)))
    out.append(("gate|up", dict(M=M, N=2 * F, K=D, mode=3, fp8=int(fp8), fold_consumer=int(fold), pf_x=pf(M, 2), **c)))
    out.append(("down", dict(M=M, N=D, K=F, mode=2, fp8=int(fp8), fold_producer=int(fold), pf_x=pf(M, 4), **c)))
    out.append(("down last layer", dict(M=M, N=D, K=F, mode=2, fp8=int(fp8), pf_x=pf(M, 4), **c)))
    out.append(("proj_out", dict(M=M, N=OUT2, K=D, mode=1, **c)))
    return out


def encoder_stack(M, d, qd, kvd, f):
    """The four projections of a layer of encoder.hip encoder_layers."""
    return [("qkv", dict(M=M, N=qd + 2 * kvd, K=d, mode=4, hn_q_cols=qd, hn_qk_cols=qd + kvd)), ("o_proj", dict(M=M, N=d, K=qd, mode=2, counters=1)),
            ("gate|up", dict(M=M, N=2 * f, K=d, mode=3)), ("down", dict(M=M, N=d, K=f, mode=2, counters=1))]


def table_requests():
    rows = []
    add = lambda group, items: rows.extend((f"{group}: {n}", r) for n, r in items)
    add("one song, CFG, sampler (folded norms)", forward_core(750, 375, True))
    add("one song, CFG, plain forward", forward_core(750, 375, False))
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
