"""The set_adapters calls whose plans tests/test_adapter_plan_cpu.py pins, and an independent restatement of the rules the plan follows
(csrc/adapter_plan.h plan_adapters, through ace355_adapter_plan).  The restatement is written from include/ace355.h and the comments of
the device structs, not from the planner:

  * a target [rows, cols] is cut into 64 x 128 tiles, ceil(rows / 64) x ceil(cols / 128) of them, column tiles fastest; the targets of
    one launch own consecutive tile ranges from 0 in target order; a decomposed factor's product is cut the same way;
  * targets appear in the order the call first mentions them with a live term (LoRA terms, then Kronecker terms, then DoRA terms;
    scale 0 drops an additive term, multiplier 0 a DoRA term), then the applied targets the call no longer names, in name order;
  * a target with a live Kronecker term is formed by the Kronecker kernel, one with a live LoRA term by the LoRA kernel; a target without
    a live additive term (restored, or DoRA over terms at scale 0) rides with the Kronecker launch when the call has a live Kronecker
    term anywhere and with the LoRA launch otherwise; a live DoRA term moves its target to the two-pass launches of that kernel;
  * every decomposed factor owns ceil4(rows x cols) floats of the factor scratch, in term order (W1 before W2); every DoRA target owns
    ceil16(8 n ntiles) bytes of partials and then ceil16(4 n) bytes of factors in the DoRA scratch, in target order, where n = rows
    and ntiles = column tiles (per output row) or n = cols and ntiles = row tiles (per input column);
  * the table holds nine sections in a fixed order, each starting on a multiple of 256 bytes, an empty one of 0 bytes;
  * launches, in order: LoRA plain, Kronecker factors, Kronecker plain, LoRA pass 1, Kronecker pass 1, DoRA factors of the LoRA-formed
    targets, of the Kronecker-formed ones, LoRA pass 2, Kronecker pass 2; a launch without entries is absent.  The Kronecker merges ask
    for the largest LDS need among the call's live Kronecker terms; the DoRA factor launches are (ceil(max n / 256), targets).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _lokr_cases as L  # noqa: E402

KINDS = tuple(k + ".weight" for k in L.KINDS)
TINY = (256, 768, 2, 2, 1, 128, 128, 2, 192, 64, 1e-6, 1e6, 1)          # the adapter tests' tiny configuration (L.TINY)
DEFAULT = (2048, 6144, 24, 16, 8, 128, 128, 2, 192, 64, 1e-6, 1e6, 0)   # include/ace355.h ace355_dit_config
TM, TN = 64, 128
LDS_MAX = 64 * 132 + 64
ROW_BYTES = {"lora_targets": 64, "lora_terms": 24, "kron_targets": 64, "kron_terms": 48, "kron_factors": 48, "dora_lora_targets": 64,
             "dora_lora_rows": 48, "dora_kron_targets": 64, "dora_kron_rows": 48}   # sizeof of the device structs (LP64)
SECTIONS = tuple(ROW_BYTES)
A_PTR, B_PTR, G_PTR = 0x10000, 0x20000, 0x30000   # device pointers are numbers to the plan
W_ALIGNED, W_ODD = 0x40000, 0x40002               # a w2 that is / is not 16-byte aligned


def ceil(a, b):
    return -(-a // b)


def name(layer, kind):
    return f"layers.{layer}.{KINDS[kind] if isinstance(kind, int) else kind + '.weight'}"


def shape(cfg, n):
    """[out, in] of a target name, None where it is none."""
    hidden, inter, layers, heads, kv_heads = cfg[:5]
    parts = n.split(".", 2)
    if len(parts) != 3 or parts[0] != "layers" or not parts[1].isdigit() or str(int(parts[1])) != parts[1] or int(parts[1]) >= layers:
        return None
    q, kv = heads * 128, kv_heads * 128
    table = {"q_proj": (q, hidden), "k_proj": (kv, hidden), "v_proj": (kv, hidden), "o_proj": (hidden, q),
             "gate_proj": (inter, hidden), "up_proj": (inter, hidden), "down_proj": (hidden, inter)}
    return table[parts[2].split(".")[1]] if parts[2] in KINDS else None


# ---------------------------------------------------------------- term rows (the fields of native.LoraTermC / KronTermC / DoraTermC)
def lora(n, rank=8, scale=1.0, a=A_PTR, b=B_PTR):
    return (n.encode() if n is not None else None, a, b, rank, scale)


def kron(cfg, n, split, scale=1.0, w2=W_ALIGNED):
    """split: (out_l, in_m, r1, r2) of tests/_lokr_cases.py, or "full"."""
    rows, cols = shape(cfg, n)
    out_l, in_m, r1, r2 = (rows, cols, 0, 0) if split == "full" else split
    f1 = (A_PTR, 0, 0) if r1 == 0 else (0, A_PTR, B_PTR)
    f2 = (w2, 0, 0) if r2 == 0 else (0, A_PTR, B_PTR)
    return (n.encode(), *f1, *f2, out_l, rows // out_l, in_m, cols // in_m, r1, r2, scale)


def dora(n, per_input=0, eps=2.0 ** -7, m=1.0, g=G_PTR):
    return (n.encode() if n is not None else None, g, per_input, eps, m)


# ---------------------------------------------------------------- the restatement
def lds_floats(out_k, in_n):
    a, b = min(out_k, TM), min(in_n, TN)
    nl = TM // a if TM % a == 0 and out_k <= TM else (TM - 1) // a + 2
    nm = TN // b if TN % b == 0 and in_n <= TN else (TN - 1) // b + 2
    return ceil(nl * nm, 4) * 4 + a * (b + 4 if b % 4 == 0 else b | 1)


def expect(cfg, lora_rows=(), kron_rows=(), dora_rows=(), applied=()):
    """What native.adapter_plan returns for a VALID call, from the rules of the module docstring."""
    order, live = [], {}

    def entry(n):
        if n not in live:
            live[n] = {"lora": [], "kron": [], "dora": None}
            order.append(n)
        return live[n]
    for t in lora_rows:
        if t[4] != 0:
            entry(t[0].decode())["lora"].append(t)
    for t in kron_rows:
        if t[13] != 0:
            entry(t[0].decode())["kron"].append(t)
    for t in dora_rows:
        if t[4] != 0:
            entry(t[0].decode())["dora"] = t
    n_merged = len(order)
    for n in sorted(set(applied)):
        if n not in live:
            entry(n)
    any_kron = any(live[n]["kron"] for n in order)
    targets, kron_out, factors, dora_out = [], [], [], {"dora_lora": [], "dora_kron": []}
    count = {c: 0 for c in ("lora", "kron", "dora_lora", "dora_kron")}
    tiles = dict(count)
    n_lora_terms = ftiles = kfloats = dbytes = max_n = 0
    lds = 4

    def product(rows, cols, rank):
        nonlocal ftiles, kfloats
        factors.append({"rows": rows, "cols": cols, "rank": rank, "tile0": ftiles, "tiles_n": ceil(cols, TN), "offset": 4 * kfloats})
        ftiles += ceil(rows, TM) * ceil(cols, TN)
        kfloats += ceil(rows * cols, 4) * 4
        return factors[-1]["offset"]
    for i, n in enumerate(order):
        e, (rows, cols) = live[n], shape(cfg, n)
        by_kron = bool(e["kron"]) or (not e["lora"] and any_kron)
        cls = ("dora_" if e["dora"] else "") + ("kron" if by_kron else "lora")
        t = {"name": n, "cls": cls, "row": count[cls], "rows": rows, "cols": cols, "tile0": tiles[cls], "tiles_n": ceil(cols, TN),
             "term0": len(kron_out) if by_kron else n_lora_terms, "nterms": len(e["kron"] if by_kron else e["lora"]),
             "restored": int(i >= n_merged)}
        count[cls] += 1
        tiles[cls] += ceil(rows, TM) * ceil(cols, TN)
        if e["dora"]:
            _n, _g, per_input, eps, m = e["dora"]
            nn, nt = (cols, ceil(rows, TM)) if per_input else (rows, ceil(cols, TN))
            part = dbytes
            dbytes += ceil(8 * nn * nt, 16) * 16
            dora_out[cls].append({"cls": cls, "per_input": per_input, "n": nn, "ntiles": nt, "eps": eps, "multiplier": m,
                                  "part_offset": part, "f_offset": dbytes})
            dbytes += ceil(4 * nn, 16) * 16
            max_n = max(max_n, nn)
        if by_kron:
            for k in e["kron"]:
                w2, out_l, out_k, in_m, in_n, r1, r2, scale = k[4], *k[7:14]
                o1 = product(out_l, in_m, r1) if r1 else -1
                o2 = product(out_k, in_n, r2) if r2 else -1
                kron_out.append({"out_l": out_l, "out_k": out_k, "in_m": in_m, "in_n": in_n,
                                 "wide": int(in_n % 8 == 0 and in_n <= TN and (r2 > 0 or w2 % 16 == 0)), "w1_f32": int(r1 > 0),
                                 "w2_f32": int(r2 > 0), "scale": scale, "w1_offset": o1, "w2_offset": o2})
                lds = max(lds, lds_floats(out_k, in_n))
        else:
            n_lora_terms += len(e["lora"])
        targets.append(t)
    rows_of = {"lora_targets": count["lora"], "lora_terms": n_lora_terms, "kron_targets": count["kron"], "kron_terms": len(kron_out),
               "kron_factors": len(factors), "dora_lora_targets": count["dora_lora"], "dora_lora_rows": count["dora_lora"],
               "dora_kron_targets": count["dora_kron"], "dora_kron_rows": count["dora_kron"]}
    sections, at = {}, 0
    for s in SECTIONS:
        sections[s] = (at, rows_of[s] * ROW_BYTES[s])
        at += ceil(rows_of[s] * ROW_BYTES[s], 256) * 256
    launches = []

    def merge(kernel, cls, pas):
        if count[cls]:
            launches.append({"kernel": kernel, "pass": pas, "entries": count[cls], "grid_x": tiles[cls], "grid_y": 1,
                             "lds_bytes": 4 * lds if kernel == "kron_merge" else 0,
                             "sections": [cls + "_targets", kernel[:4] + "_terms", cls + "_rows" if pas else None]})

    def dora_factors(cls):
        if count[cls]:
            launches.append({"kernel": "dora_factors", "pass": 0, "entries": count[cls], "grid_x": ceil(max_n, 256), "grid_y": count[cls],
                             "lds_bytes": 0, "sections": [cls + "_rows", None, None]})
    merge("lora_merge", "lora", 0)
    if factors:
        launches.append({"kernel": "kron_factors", "pass": 0, "entries": len(factors), "grid_x": ftiles, "grid_y": 1, "lds_bytes": 0,
                         "sections": ["kron_factors", None, None]})
    merge("kron_merge", "kron", 0)
    merge("lora_merge", "dora_lora", 1)
    merge("kron_merge", "dora_kron", 1)
    dora_factors("dora_lora")
    dora_factors("dora_kron")
    merge("lora_merge", "dora_lora", 2)
    merge("kron_merge", "dora_kron", 2)
    cross = [n.split(".")[2:4] for n in order]
    return {"n_targets": len(order), "n_merged": n_merged, "n_launches": len(launches), "n_lora_terms": n_lora_terms,
            "n_kron_terms": len(kron_out), "n_factors": len(factors), "n_dora": count["dora_lora"] + count["dora_kron"],
            "stale_kv": int(any(c in (["cross_attn", "k_proj"], ["cross_attn", "v_proj"]) for c in cross)),
            "stale_o": int(["cross_attn", "o_proj"] in cross),
            "table_bytes": at if order else 0, "kscratch_floats": kfloats, "dscratch_bytes": dbytes,
            "sections": sections if order else {s: (0, 0) for s in SECTIONS}, "targets": targets, "launches": launches, "kron": kron_out,
            "factors": factors, "dora": dora_out["dora_lora"] + dora_out["dora_kron"]}


# ---------------------------------------------------------------- the calls
Q0, K0, UP0, DOWN0 = L.SHAPE_TARGETS   # 256 x 256, 128 x 256, 768 x 256, 256 x 768
XK1, XO1, V1 = name(1, "cross_attn.k_proj"), name(1, "cross_attn.o_proj"), name(1, "self_attn.v_proj")


def _split_call(split):
    return [kron(TINY, n, split) for n in L.SHAPE_TARGETS if L.split_fits(shape(TINY, n), split)]


def _all_kinds(cfg, layers, split=(8, 8, 0, 8)):
    return [kron(cfg, name(li, k), split) for li in range(layers) for k in range(len(KINDS))]


def _default_lokr():
    def near_square(n):
        a = int(n ** 0.5)
        while n % a:
            a -= 1
        return a, n // a
    out = []
    for li in range(DEFAULT[2]):
        for k in range(len(KINDS)):
            n = name(li, k)
            (out_l, out_k), (in_m, in_n) = (near_square(d) for d in shape(DEFAULT, n))
            out.append(kron(DEFAULT, n, (out_l, in_m, 0, 64 if 64 < max(out_k, in_n) / 2 else 0)))
    return out


# (label, cfg, lora, kron, dora, applied)
CASES = [
    ("empty call, nothing applied", TINY, [], [], [], []),
    ("empty call, targets applied: restore only", TINY, [], [], [], [UP0, Q0, XO1]),
    ("LoRA only: two terms on one target, one term at scale 0", TINY,
     [lora(Q0), lora(K0, rank=3), lora(Q0, rank=70, scale=0.5), lora(UP0, scale=0.0)], [], [], [UP0]),
] + [(f"Kronecker only, split {s}", TINY, [], _split_call(s), [], []) for s in L.SPLITS] + [
    ("Kronecker: an unaligned w2, a second term, a term at scale 0", TINY, [],
     [kron(TINY, Q0, (16, 16, 0, 0), w2=W_ODD), kron(TINY, Q0, (16, 64, 0, 8)), kron(TINY, K0, (16, 16, 0, 0), scale=0.0)], [], []),
    ("LoRA and Kronecker on different targets, a restored third", TINY, [lora(Q0)], [kron(TINY, DOWN0, (8, 32, 4, 40))], [], [XK1, Q0]),
    ("DoRA on a LoRA target, per output row", TINY, [lora(UP0)], [], [dora(UP0, 0)], []),
    ("DoRA on a Kronecker target, per input column", TINY, [], [kron(TINY, DOWN0, (16, 64, 0, 8))], [dora(DOWN0, 1, eps=0.0, m=0.6)], []),
    ("a DoRA term with multiplier 0", TINY, [lora(Q0)], [], [dora(Q0, 0, m=0.0)], []),
    ("a DoRA target whose additive terms are all at scale 0", TINY, [lora(Q0, scale=0.0), lora(K0)], [], [dora(Q0, 1)], []),
    ("a DoRA target over Kronecker terms at scale 0, beside a live Kronecker term", TINY, [],
     [kron(TINY, Q0, (16, 16, 0, 0), scale=0.0), kron(TINY, K0, (16, 16, 0, 0))], [dora(Q0, 0)], []),
    ("all four classes plus a restored target", TINY, [lora(Q0), lora(K0), lora(K0, rank=16)],
     [kron(TINY, UP0, (24, 16, 0, 1)), kron(TINY, DOWN0, (2, 3, 0, 64)), kron(TINY, XO1, (16, 16, 0, 0)), kron(TINY, XK1, "full")],
     [dora(K0, 0), dora(DOWN0, 1), dora(XO1, 0, eps=0.0)], [V1, Q0]),
    ("default configuration, all eleven kinds of all layers, the default LoKr split", DEFAULT, [], _default_lokr(), [], []),
    ("default configuration, all eleven kinds of all layers, DoRA on every third", DEFAULT, [], _all_kinds(DEFAULT, 24),
     [dora(name(li, k), (li + k) % 2) for li in range(24) for k in range(len(KINDS)) if (li * 11 + k) % 3 == 0], [name(3, 2)]),
]

NOT_A_TARGET = ("set_adapters: '{}' is not a LoRA target (layers.{{i}}.{{self_attn,cross_attn}}.{{q,k,v,o}}_proj.weight, "
                "layers.{{i}}.mlp.{{gate,up,down}}_proj.weight)")
INV = "invalid argument: "
BAD = "layers.2.self_attn.q_proj.weight"   # (the tiny configuration has layers 0 and 1)
_k = kron(TINY, Q0, (16, 16, 0, 0))
_kd = kron(TINY, Q0, (16, 16, 4, 8))


def _with(row, **at):
    row = list(row)
    for i, v in at.items():
        row[int(i[1:])] = v
    return tuple(row)


# (label, lora, kron, dora, message): every refusal of set_adapters_impl that does not need a handle, code ACE355_ERR_INVALID (1)
REFUSALS = [
    ("LoRA: null name", [lora(None)], [], [], INV + "set_adapters: null name / A / B"),
    ("LoRA: null A", [lora(Q0, a=0)], [], [], INV + "set_adapters: null name / A / B"),
    ("LoRA: null B", [lora(Q0, b=0)], [], [], INV + "set_adapters: null name / A / B"),
    ("LoRA: unknown name", [lora(BAD)], [], [], NOT_A_TARGET.format(BAD)),
    ("LoRA: a norm weight is no target", [lora("layers.0.self_attn.q_norm.weight")], [], [], NOT_A_TARGET.format("layers.0.self_attn.q_norm.weight")),
    ("LoRA: rank 0", [lora(Q0, rank=0)], [], [], INV + "set_adapters: rank must be >= 1 and scale finite"),
    ("LoRA: scale inf", [lora(Q0, scale=float("inf"))], [], [], INV + "set_adapters: rank must be >= 1 and scale finite"),
    ("Kronecker: null name", [], [_with(_k, _0=None)], [], INV + "set_adapters: null name in a Kronecker term"),
    ("Kronecker: unknown name", [], [_with(_k, _0=b"layers.0.mlp.gate_proj")], [], NOT_A_TARGET.format("layers.0.mlp.gate_proj")),
    ("Kronecker: negative rank", [], [_with(_k, _11=-1)], [], INV + "set_adapters: a Kronecker factor's rank must be >= 0"),
    ("Kronecker: w1 and w1a both set", [], [_with(_k, _2=A_PTR)], [],
     INV + "set_adapters: each Kronecker factor needs exactly one of {w} (rank 0) / {w_a, w_b} (rank >= 1)"),
    ("Kronecker: no w2 at all", [], [_with(_k, _4=0)], [],
     INV + "set_adapters: each Kronecker factor needs exactly one of {w} (rank 0) / {w_a, w_b} (rank >= 1)"),
    ("Kronecker: a decomposed factor with rank 0", [], [_with(_kd, _12=0)], [],
     INV + "set_adapters: each Kronecker factor needs exactly one of {w} (rank 0) / {w_a, w_b} (rank >= 1)"),
    ("Kronecker: a full factor with a rank", [], [_with(_k, _11=4)], [],
     INV + "set_adapters: each Kronecker factor needs exactly one of {w} (rank 0) / {w_a, w_b} (rank >= 1)"),
    ("Kronecker: out_l x out_k is not out", [], [_with(_k, _7=8)], [],
     INV + "set_adapters: out_l x out_k / in_m x in_n do not give the target's [out, in]"),
    ("Kronecker: in_n 0", [], [_with(_k, _10=0)], [], INV + "set_adapters: out_l x out_k / in_m x in_n do not give the target's [out, in]"),
    ("Kronecker: scale nan", [], [_with(_k, _13=float("nan"))], [], INV + "set_adapters: scale must be finite"),
    ("a target named by both families", [lora(Q0, scale=0.0)], [_k], [], f"set_adapters: '{Q0}' is named by a LoRA term and by a Kronecker term"),
    ("DoRA: null name", [lora(Q0)], [], [dora(None)], INV + "set_adapters: null name / g in a DoRA term"),
    ("DoRA: null g", [lora(Q0)], [], [dora(Q0, g=0)], INV + "set_adapters: null name / g in a DoRA term"),
    ("DoRA: unknown name", [lora(Q0)], [], [dora(BAD)], NOT_A_TARGET.format(BAD)),
    ("DoRA: per_input 2", [lora(Q0)], [], [dora(Q0, per_input=2)], INV + "set_adapters: a DoRA term's per_input must be 0 or 1"),
    ("DoRA: negative eps", [lora(Q0)], [], [dora(Q0, eps=-1.0)],
     INV + "set_adapters: a DoRA term's eps must be finite and >= 0 and its multiplier finite"),
    ("DoRA: multiplier inf", [lora(Q0)], [], [dora(Q0, m=float("inf"))],
     INV + "set_adapters: a DoRA term's eps must be finite and >= 0 and its multiplier finite"),
    ("DoRA: two terms on one target", [lora(Q0)], [], [dora(Q0, m=0.0), dora(Q0)], f"set_adapters: two DoRA terms name '{Q0}'"),
    ("DoRA: no additive term beside it", [lora(Q0)], [], [dora(K0)],
     f"set_adapters: the DoRA term on '{K0}' has no LoRA / Kronecker term beside it in this call"),
]
# refusals that the tiny configuration cannot reach: (label, cfg, lora, kron, dora, message)
WIDE = (256, 772, 1, 2, 1, 128, 128, 2, 192, 64, 1e-6, 1e6, 0)   # intermediate 772: down_proj has 772 columns
REFUSALS_CFG = [
    ("target columns not a multiple of 8", WIDE, [lora("layers.0.mlp.down_proj.weight")], [], [],
     INV + "set_adapters: target columns must be a multiple of 8"),
]
