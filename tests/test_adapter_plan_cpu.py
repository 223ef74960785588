"""CPU: the adapter merge plan (csrc/adapter_plan.h plan_adapters, through ace355_adapter_plan) - which targets, table sections, scratch
regions and launches a set_adapters call comes to.  Every field is compared with the independent restatement of
tests/_adapter_plan_cases.py; the structural conditions a kernel relies on are asserted on their own; every refusal that needs no handle
is pinned by code and message; and the same calls plus a seeded random sweep run through tests/adapter_plan_sweep.cpp, a stand-alone
program built with the host compiler under AddressSanitizer and UBSan that fills the table and touches every scratch region.
(Not reachable, so not pinned: "Kronecker split exceeds the merge tile's LDS" - lokr_lds_floats stays below the limit for every split.
The refusals of an unfinalized handle and of a quantised one need a handle: the GPU tests of the three families.)"""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

import _adapter_plan_cases as cases
from ace355 import native


def f32(x):
    return ctypes.c_float(x).value


def plan(cfg, lora, kron, dora, applied):
    return native.adapter_plan(native.DitConfigC(*cfg), lora, kron, dora, applied)


def rounded(e):
    """The restatement with its floats as the C ABI carries them."""
    for r in e["kron"]:
        r["scale"] = f32(r["scale"])
    for r in e["dora"]:
        r["eps"], r["multiplier"] = f32(r["eps"]), f32(r["multiplier"])
    return e


IDS = [c[0] for c in cases.CASES]


@pytest.mark.parametrize("case", cases.CASES, ids=IDS)
def test_plan_matches_the_restatement(case):
    _label, cfg, lora, kron, dora, applied = case
    got, exp = plan(cfg, lora, kron, dora, applied), rounded(cases.expect(cfg, lora, kron, dora, applied))
    assert set(got) == set(exp)
    for key in exp:
        if isinstance(exp[key], list):
            assert len(got[key]) == len(exp[key]), key
            for i, (g, e) in enumerate(zip(got[key], exp[key])):
                assert g == e, (key, i)
        else:
            assert got[key] == exp[key], key


def _disjoint(regions, what):
    regions = sorted(r for r in regions if r[1] > 0)
    for (a, n), (b, _m) in zip(regions, regions[1:]):
        assert a + n <= b, (what, a, n, b)


@pytest.mark.parametrize("case", cases.CASES, ids=IDS)
def test_plan_structure(case):
    _label, cfg, lora, kron, dora, applied = case
    p = plan(cfg, lora, kron, dora, applied)
    # every target of the call exactly once, in exactly one class
    live = [t[0].decode() for t in lora if t[4] != 0] + [t[0].decode() for t in kron if t[13] != 0] + [t[0].decode() for t in dora if t[4] != 0]
    names = [t["name"] for t in p["targets"]]
    assert len(names) == len(set(names)) and set(names) == set(live) | set(applied)
    assert names[:p["n_merged"]] == list(dict.fromkeys(live)), "first-mention order"
    assert names[p["n_merged"]:] == sorted(set(applied) - set(live)) and all(t["restored"] == (i >= p["n_merged"]) for i, t in enumerate(p["targets"]))
    by_cls = {c: [t for t in p["targets"] if t["cls"] == c] for c in native.ADAPTER_CLASSES}
    for c, ts in by_cls.items():
        assert [t["row"] for t in ts] == list(range(len(ts)))
        at = 0
        for t in ts:   # tile ranges contiguous from 0
            assert t["tile0"] == at and t["tiles_n"] == cases.ceil(t["cols"], 128) and t["cols"] % 8 == 0
            at += cases.ceil(t["rows"], 64) * t["tiles_n"]
        for l in p["launches"]:
            if l["sections"][0] == c + "_targets":
                assert l["grid_x"] == at and l["entries"] == len(ts) and l["grid_y"] == 1
        assert any(l["sections"][0] == c + "_targets" for l in p["launches"]) == bool(ts)
    # term ranges partition the term rows, in target order
    for family, total in (("lora", p["n_lora_terms"]), ("kron", p["n_kron_terms"])):
        at = 0
        for t in p["targets"]:
            if t["cls"].endswith(family):
                assert t["term0"] == at
                at += t["nterms"]
        assert at == total
    at = 0
    for f in p["factors"]:
        assert f["tile0"] == at and f["tiles_n"] == cases.ceil(f["cols"], 128) and f["rank"] >= 1
        at += cases.ceil(f["rows"], 64) * f["tiles_n"]
    assert [l["grid_x"] for l in p["launches"] if l["kernel"] == "kron_factors"] == ([at] if p["factors"] else [])
    # the table
    secs = p["sections"]
    for s, (a, n) in secs.items():
        assert a % 256 == 0 and a + n <= p["table_bytes"] and n % cases.ROW_BYTES[s] == 0, s
    _disjoint(secs.values(), "table sections")
    for l in p["launches"]:
        assert secs[l["sections"][0]][1] == l["entries"] * cases.ROW_BYTES[l["sections"][0]]
        if l["pass"]:
            assert secs[l["sections"][2]][1] == l["entries"] * cases.ROW_BYTES[l["sections"][2]], "one DoRA row per target of a DoRA launch"
        if l["kernel"] == "kron_merge":
            assert 4 * 4 <= l["lds_bytes"] <= 4 * cases.LDS_MAX and l["lds_bytes"] >= 4 * max(cases.lds_floats(k["out_k"], k["in_n"]) for k in p["kron"] or [{"out_k": 1, "in_n": 1}])
        else:
            assert l["lds_bytes"] == 0
    # the scratch regions
    kregions = [(f["offset"], 4 * f["rows"] * f["cols"]) for f in p["factors"]]
    assert all(a % 16 == 0 and a + n <= 4 * p["kscratch_floats"] for a, n in kregions)
    _disjoint(kregions, "factor scratch")
    assert sorted(k[o] for k in p["kron"] for o in ("w1_offset", "w2_offset") if k[o] >= 0) == sorted(f["offset"] for f in p["factors"])
    dregions = [r for d in p["dora"] for r in ((d["part_offset"], 8 * d["n"] * d["ntiles"]), (d["f_offset"], 4 * d["n"]))]
    assert all(a % 16 == 0 and a + n <= p["dscratch_bytes"] for a, n in dregions)
    _disjoint(dregions, "DoRA scratch")
    for l in p["launches"]:
        if l["kernel"] == "dora_factors":
            assert 256 * l["grid_x"] >= max(d["n"] for d in p["dora"]) and l["grid_y"] == l["entries"]
    # launch order
    rank = {("lora_merge", 0): 0, ("kron_factors", 0): 1, ("kron_merge", 0): 2, ("lora_merge", 1): 3, ("kron_merge", 1): 4,
            ("dora_factors", 0): 5, ("lora_merge", 2): 7, ("kron_merge", 2): 8}
    seq = [rank[(l["kernel"], l["pass"])] + (l["kernel"] == "dora_factors" and l["sections"][0] == "dora_kron_rows") for l in p["launches"]]
    assert seq == sorted(set(seq))


def test_cases_reach_every_class_and_launch():
    seen_cls, seen_launch, wide = set(), set(), set()
    for _label, cfg, lora, kron, dora, applied in cases.CASES:
        p = plan(cfg, lora, kron, dora, applied)
        seen_cls |= {(t["cls"], t["restored"]) for t in p["targets"]}
        seen_launch |= {(l["kernel"], l["pass"], l["sections"][0]) for l in p["launches"]}
        wide |= {(k["wide"], k["w1_f32"], k["w2_f32"]) for k in p["kron"]}
    assert seen_cls >= set(itertools.product(native.ADAPTER_CLASSES, (0,))) | {("lora", 1), ("kron", 1)}
    assert len(seen_launch) == 9
    assert wide >= {(1, 0, 0), (0, 0, 0), (1, 0, 1), (0, 0, 1), (1, 1, 1)}


@pytest.mark.parametrize("case", [(c[0], cases.TINY, *c[1:]) for c in cases.REFUSALS] + cases.REFUSALS_CFG, ids=lambda c: c[0])
def test_refusals_keep_code_and_message(case):
    _label, cfg, lora, kron, dora, message = case
    with pytest.raises(RuntimeError) as e:
        plan(cfg, lora, kron, dora, [cases.UP0])
    assert str(e.value) == f"ace355 native call failed (adapter_plan, code 1): {message}"


@pytest.mark.parametrize("which, message", [(0, "set_adapters: terms"), (1, "set_adapters: kron terms"), (2, "set_adapters: dora terms")])
def test_refusals_of_the_term_arrays(which, message):
    lib, C = native.lib(), ctypes
    cfg, rows, info = native.DitConfigC(*cases.TINY), native.AdapterPlanRowsC(), native.AdapterPlanInfoC()
    one = ((native.LoraTermC * 1)(), (native.KronTermC * 1)(), (native.DoraTermC * 1)())
    for n, arr in ((-1, one[which]), (1, None)):   # a negative count; a count without an array
        args = [one[0], 0, one[1], 0, one[2], 0]
        args[2 * which], args[2 * which + 1] = arr, n
        assert lib.ace355_adapter_plan(C.byref(cfg), *args, None, 0, C.byref(rows), C.byref(info)) == 1
        assert native.last_error() == "invalid argument: " + message
    assert lib.ace355_adapter_plan(C.byref(cfg), one[0], 0, one[1], 0, one[2], 0, (C.c_char_p * 1)(b"layers.9.mlp.up_proj.weight"), 1,
                                   C.byref(rows), C.byref(info)) == 1
    assert native.last_error() == "invalid argument: adapter_plan: an applied name is not a target"


def test_null_handle_refusal_of_the_three_entry_points():
    lib, one = native.lib(), ((native.LoraTermC * 1)(), (native.KronTermC * 1)(), (native.DoraTermC * 1)())
    for rc in (lib.ace355_dit_set_adapters(None, one[0], 0, None), lib.ace355_dit_set_adapters_mixed(None, one[0], 0, one[1], 0, None),
               lib.ace355_dit_set_adapters_dora(None, one[0], 0, one[1], 0, one[2], 0, None)):
        assert rc == 1 and native.last_error() == "invalid argument: set_adapters: null handle"


def test_three_entry_points_are_one_plan():
    """n_kron 0 IS set_adapters and n_dora 0 IS set_adapters_mixed: the plan has no input but the term arrays, so empty arrays are the
    narrower entry points, and a LoRA-only call launches the LoRA merge alone."""
    p = plan(cases.TINY, [cases.lora(cases.Q0), cases.lora(cases.K0)], [], [], [cases.UP0])
    assert [(l["kernel"], l["pass"]) for l in p["launches"]] == [("lora_merge", 0)] and p["kscratch_floats"] == p["dscratch_bytes"] == 0
    p = plan(cases.TINY, [cases.lora(cases.Q0)], [cases.kron(cases.TINY, cases.K0, (16, 16, 0, 0))], [], [cases.UP0])
    assert [(l["kernel"], l["pass"]) for l in p["launches"]] == [("lora_merge", 0), ("kron_merge", 0)] and p["dscratch_bytes"] == 0
    assert [t["cls"] for t in p["targets"]] == ["lora", "kron", "kron"], "beside a live Kronecker term the restored target rides with it"


# ---------------------------------------------------------------- the same calls, and a random sweep, under host sanitizers
def _sweep_input(path):
    def ref(cfg, n):
        s = cases.shape(cfg, n) if isinstance(n, str) else None
        if s is None:
            return "-1 0 0 0"
        li, kind = int(n.split(".")[1]), cases.KINDS.index(n.split(".", 2)[2])
        return f"{li * 11 + kind} {s[0]} {s[1]} {1 if kind in (5, 6) else 2 if kind == 7 else 0}"

    def nm(b):
        return b.decode() if b is not None else "-"
    calls = [(c[1], c[2], c[3], c[4], c[5], 0) for c in cases.CASES] + [(cases.TINY, c[1], c[2], c[3], [cases.UP0], 1) for c in cases.REFUSALS] + \
        [(c[1], c[2], c[3], c[4], [], 1) for c in cases.REFUSALS_CFG]
    with open(path, "w") as f:
        for cfg, lora, kron, dora, applied, code in calls:
            e = cases.expect(cfg, lora, kron, dora, applied) if code == 0 else None
            f.write(f"call {len(lora)} {len(kron)} {len(dora)} {len(applied)} {code} " +
                    (f"{e['n_targets']} {e['n_launches']} {e['table_bytes']} {e['kscratch_floats']} {e['dscratch_bytes']}\n" if e else "0 0 0 0 0\n"))
            for t in lora:
                f.write(f"L {ref(cfg, nm(t[0]))} {nm(t[0])} {t[1]} {t[2]} {t[3]} {t[4]!r}\n")
            for t in kron:
                f.write(f"K {ref(cfg, nm(t[0]))} {nm(t[0])} " + " ".join(str(x) for x in t[1:13]) + f" {t[13]!r}\n")
            for t in dora:
                f.write(f"D {ref(cfg, nm(t[0]))} {nm(t[0])} {t[1]} {t[2]} {t[3]!r} {t[4]!r}\n")
            for n in sorted(set(applied)):
                f.write(f"A {ref(cfg, n)} {n}\n")


def test_sweep_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe, inp = tmp_path / "adapter_plan_sweep", tmp_path / "calls.txt"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(cases.ROOT, "tests", "adapter_plan_sweep.cpp"), "-o", str(exe)], check=True)
    _sweep_input(inp)
    r = subprocess.run([str(exe), str(inp), "20000"], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    n = len(cases.CASES) + len(cases.REFUSALS) + len(cases.REFUSALS_CFG)
    assert f"{n} listed calls as expected" in r.stdout and "20000 random calls" in r.stdout
