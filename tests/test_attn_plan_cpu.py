"""CPU: the attention launch plan (csrc/attn_plan.h plan_attention, through ace355_attn_plan) - which kernel instantiation, grid and
split-KV part count every attention launch of the project gets.  A committed table pins the shapes the product and the GPU tests launch,
fresh processes pin what each ACE355_ATTN_* switch does to it, and a sweep checks the conditions attn_plan.h states in comments."""
import json
import os
import subprocess
import sys

import pytest

import _attn_plan_cases as cases


@pytest.fixture(scope="module")
def table():
    import ace355  # noqa: F401
    return json.load(open(cases.TABLE))


def _diff(got, want):
    return {k: (got.get(k), want.get(k)) for k in sorted(set(got) | set(want)) if got.get(k) != want.get(k)}


def _form(p):
    return (p["kernel"], p["nw"])


def test_plans_match_the_committed_table(table):
    """tests/attn_plan_table.json, field by field.  A deliberate change of the heuristics regenerates it
    (python tests/_attn_plan_cases.py --write); its diff then shows which shapes moved."""
    now = cases.table_requests()
    assert [r["name"] for r in table] == [n for n, _r in now], "the table's rows are not the requests of tests/_attn_plan_cases.py: regenerate it"
    bad = []
    for row, (name, rq) in zip(table, now):
        if row["request"] != rq:
            bad.append(f"{name}: request {_diff(rq, row['request'])}")
        d = _diff(cases.plan(rq), row["plan"])
        if d:
            bad.append(f"{name}: (got, table) {d}")
    print("\n".join(bad))
    assert not bad, f"{len(bad)} rows differ from the table"


def test_the_gpu_test_rows_reach_every_kernel_form_and_split(table):
    """test_attention's rows are in the regime each names, and together (with the one-order row) they run every instantiation
    plan_attention can emit and every part count of the split-KV heuristic."""
    from ace355 import native
    by_name = {r["name"]: r["plan"] for r in table}
    forms, splits = set(), set()
    for shape, (kernel, nw, kv_split) in cases.ATTENTION_ROWS:
        p = by_name[f"test_attention: {shape}"]
        assert (p["kernel"], p["nw"], p["kv_split"]) == (kernel, nw, kv_split), (shape, p)
        forms.add((kernel, nw))
        splits.add(kv_split)
    shape, (kernel, nw, kv_split) = cases.ONE_ORDER_ROW
    prev = native.gemm_set_k_rotation(0)
    try:
        p = cases.plan(cases.request(shape, part_floats=cases.PART))
    finally:
        native.gemm_set_k_rotation(prev)
    assert (p["kernel"], p["nw"], p["kv_split"]) == (kernel, nw, kv_split), p
    forms.add((kernel, nw))
    assert forms == cases.ALL_FORMS and splits == cases.ALL_SPLITS, (forms, splits)


def test_the_key_rows_reach_every_form_band_split_mask_and_workgroup_order(table):
    """tests/test_attention_keys_gpu.py's rows take the launches they name, and together they run every instantiation full AND banded,
    every part count of the split-KV heuristic and a banded split, a key-padding mask on every kernel, and all three arms of the GQA-family
    kernels' workgroup decode (Hkv = 8, a larger multiple of 8, no multiple of 8) on both of them."""
    by_name = {r["name"]: r["plan"] for r in table}
    forms, splits, masked, decode = set(), set(), set(), set()
    for row in cases.KEY_ROWS:
        shape, (kernel, nw, kv_split), opts = row
        p = cases.key_row_plan(row)
        assert (p["kernel"], p["nw"], p["kv_split"]) == (kernel, nw, kv_split), (row, p)
        if "krot" not in opts:
            assert p == by_name[f"test_attention_keys: {shape}{' masked' if 'lens' in opts else ''}"], row
        N, Sq, Skv, Hq, Hkv, window = shape
        forms.add((kernel, nw, window >= 0))
        splits.add((kv_split, window >= 0))
        if "lens" in opts:
            lens = opts["lens"]
            assert Sq == Skv and len(lens) == N and Skv in lens and 0 in lens and any(x % 64 for x in lens), row
            # banded: the later queries of some live sequence have no visible key
            assert window < 0 or any(0 < x and x + window < Sq - 1 for x in lens), row
            masked.add((kernel, nw))
        if kernel != "attn3":
            assert Hq == 2 * Hkv
            decode.add((kernel, "generic" if Hkv % 8 else f"hg{Hkv // 8}"))
            if Hkv % 8:   # surplus workgroups of the padded grid have to leave
                assert p["grid_x"] > N * Hkv * -(-Sq // (32 * nw)), row
    assert forms == {(k, n, b) for k, n in cases.ALL_FORMS for b in (False, True)}, forms
    assert {s for s, _b in splits} == cases.ALL_SPLITS and any(s > 1 and b for s, b in splits), splits
    assert {k for k, _n in masked} == {"attn3", "gqa", "rot"} and masked >= {("attn3", 4), ("gqa", 3), ("gqa", 4), ("gqa", 6), ("rot", 3)}, masked
    assert decode == {(k, d) for k in ("gqa", "rot") for d in ("hg1", "hg2", "generic")}, decode


# ---------------------------------------------------------------------------------------------- knobs: read once, so fresh processes
def _spawn(env=None, krot=None):
    cmd = [sys.executable, os.path.join(cases.ROOT, "tests", "_attn_plan_cases.py"), "--plans"] + ([] if krot is None else ["--krot", str(krot)])
    clean = {k: v for k, v in os.environ.items() if not k.startswith("ACE355_")}
    return subprocess.Popen(cmd, env={**clean, **(env or {})}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


KNOB_CASES = [("ACE355_ATTN_GQA", "0"), ("ACE355_ATTN_GQA", "3"), ("ACE355_ATTN_GQA", "4"), ("ACE355_ATTN_GQA", "6"), ("ACE355_ATTN_ROT", "0"),
              ("ACE355_ATTN_ROT", "2"), ("ACE355_ATTN_NW", "4"), ("ACE355_ATTN_NW", "8"), ("ACE355_ATTN_KVSPLIT", "1"), ("ACE355_ATTN_KVSPLIT", "2"),
              ("ACE355_ATTN_KVSPLIT", "4"), ("ACE355_ATTN_KVSPLIT", "8"),
              ("ACE355_ATTN_DEFER", "0"), ("ACE355_ATTN_CLK", "1"), ("ACE355_MAX_WGS", "128"), ("krot", "0"), ("krot", "1"), ("krot", "2")]


@pytest.fixture(scope="module")
def knob_plans():
    """(knob, value) -> that process's rows; six processes at a time."""
    out = {}
    for i in range(0, len(KNOB_CASES), 6):
        procs = {(k, v): (_spawn(krot=int(v)) if k == "krot" else _spawn({k: v})) for k, v in KNOB_CASES[i:i + 6]}
        for key, p in procs.items():
            so, se = p.communicate(timeout=300)
            assert p.returncode == 0, (key, se[-2000:])
            out[key] = json.loads(so)
    return out


def _rows(knob_plans, table, knob, value):
    """(request, default plan, this knob's plan)"""
    rows = knob_plans[(knob, value)]
    assert [r["name"] for r in rows] == [r["name"] for r in table]
    return [(t["request"], t["plan"], r["plan"]) for t, r in zip(table, rows)]


def test_knob_gqa(knob_plans, table):
    rows = _rows(knob_plans, table, "ACE355_ATTN_GQA", "0")
    assert all(p["kernel"] == "attn3" and not p["mx_out_ok"] for _rq, _d, p in rows) and any(d["kernel"] != "attn3" for _rq, d, _p in rows)
    for nwh in (3, 4, 6):   # pinned wherever Hq == 2 Hkv; at 96 rows the key-split kernel takes over unless MXFP8 output is asked for
        for rq, _d, p in _rows(knob_plans, table, "ACE355_ATTN_GQA", str(nwh)):
            if rq["Hq"] != 2 * rq["Hkv"]:
                assert p["kernel"] == "attn3", (rq, p)
            else:
                assert _form(p) == (("rot", 3) if nwh == 3 and not rq.get("mx_out") else ("gqa", nwh)), (rq, p)
                assert p["grid_x"] == -(-rq["N"] * rq["Hkv"] * -(-rq["Sq"] // (32 * p["nw"])) // 8) * 8 and p["threads"] == (768 if p["kernel"] == "rot" else 128 * nwh)


def test_knob_rot(knob_plans, table):
    rows = _rows(knob_plans, table, "ACE355_ATTN_ROT", "0")
    assert all(p["kernel"] != "rot" for _rq, _d, p in rows) and any(d["kernel"] == "rot" for _rq, d, _p in rows)
    assert all(_form(p) == ("gqa", 3) if d["kernel"] == "rot" else p == d for _rq, d, p in rows)
    rows = _rows(knob_plans, table, "ACE355_ATTN_ROT", "2")
    assert any(d["kernel"] == "gqa" and p["kernel"] == "rot" for _rq, d, p in rows)
    for rq, d, p in rows:   # every GQA launch but those with MXFP8 output
        assert (_form(p) == ("rot", 3) and p["threads"] == 768) if d["kernel"] != "attn3" and not rq.get("mx_out") else p == d, (rq, p)


def test_knob_nw_and_kvsplit(knob_plans, table):
    for nw in (4, 8):
        rows = _rows(knob_plans, table, "ACE355_ATTN_NW", str(nw))
        assert all((p["nw"] == nw and p["threads"] == 64 * nw) if d["kernel"] == "attn3" else p == d for _rq, d, p in rows)
        assert any(d["kernel"] == "attn3" and d["nw"] != nw for _rq, d, _p in rows)
    assert all(p["kv_split"] == 1 for _rq, _d, p in _rows(knob_plans, table, "ACE355_ATTN_NW", "8"))   # only the 4-wave kernel splits
    rows = _rows(knob_plans, table, "ACE355_ATTN_KVSPLIT", "1")
    assert all(p["kv_split"] == 1 and p["merge_grid"] == 0 for _rq, _d, p in rows) and any(d["kv_split"] > 1 for _rq, d, _p in rows)
    # a forced part count holds wherever the split applies - the 4-wave kernel with scratch, no mask, no MXFP8 output, fewer than 128
    # workgroups walking at least 8 key tiles - and fits the scratch, also where the heuristic's own count did not fit; and nowhere else
    hit = set()
    for forced in (2, 4, 8):
        for rq, d, p in _rows(knob_plans, table, "ACE355_ATTN_KVSPLIT", str(forced)):
            N, Sq, Skv, Hq, window = rq["N"], rq["Sq"], rq["Skv"], rq["Hq"], rq["window"]
            tiles = -(-Skv // 64) if window < 0 else min(-(-Skv // 64), (128 + 2 * window + 63) // 64 + 1)
            applies = (_form(d) == ("attn3", 4) and rq.get("part_floats", 0) > 0 and not rq.get("has_kv_len") and not rq.get("mx_out")
                       and -(-Sq // 128) * Hq * N < 128 and tiles >= 8)
            want = forced if applies and forced * N * Hq * Sq * 132 <= rq["part_floats"] else 1
            assert p["kv_split"] == want and (p["merge_grid"] > 0) == (want > 1) and _form(p) == _form(d), (forced, rq, p)
            assert p["kernel"] != "attn3" or p["grid_x"] == -(-Sq // (32 * p["nw"])) * want, (forced, rq, p)
            hit.add((d["kv_split"] > 1, want > 1))
    assert hit >= {(False, False), (False, True), (True, True)}   # (heuristic splits, forced splits); (False, True): the 2 Mi-float edge row


def test_knobs_outside_the_plan_and_max_wgs(knob_plans, table):
    for knob, value in (("ACE355_ATTN_DEFER", "0"), ("ACE355_ATTN_CLK", "1")):   # kernel arguments, not launch shape
        assert all(p == d for _rq, d, p in _rows(knob_plans, table, knob, value))
    # ACE355_MAX_WGS=128 is what cu_slots = 128 asks for, request by request
    rows = _rows(knob_plans, table, "ACE355_MAX_WGS", "128")
    assert any(p != d for _rq, d, p in rows)
    for rq, _d, p in rows:
        if not rq.get("cu_slots"):
            assert p == cases.plan({**rq, "cu_slots": 128}), rq


def test_k_rotation_modes_through_the_setter(knob_plans, table):
    """Mode 0, "one summation order whatever the launch shape": no key-split kernel and no split-KV; modes 1 and 2 are the default."""
    rows = _rows(knob_plans, table, "krot", "0")
    assert any(d["kernel"] == "rot" for _rq, d, _p in rows) and any(d["kv_split"] > 1 for _rq, d, _p in rows)
    for rq, d, p in rows:
        assert p["kernel"] != "rot" and p["kv_split"] == 1 and p["merge_grid"] == 0
        assert _form(p) == (("gqa", 3) if d["kernel"] == "rot" else _form(d)) and p["mx_out_ok"] == d["mx_out_ok"]
    for mode in ("1", "2"):
        assert all(p == d for _rq, d, p in _rows(knob_plans, table, "krot", mode))


# ---------------------------------------------------------------------------------------------- invariants over a sweep
@pytest.fixture(params=[1, 0])
def k_rotation(request):
    """The sweep under the default K rotation and, through the setter, in the one-order mode."""
    from ace355 import native
    prev = native.gemm_set_k_rotation(request.param)
    yield request.param
    native.gemm_set_k_rotation(prev)


def test_invariants_over_a_sweep(k_rotation):
    """What attn_plan.h's comments promise about a plan: N 1 .. 16, Sq and Skv on both sides of the 32 NW-row block edges and the 64-key
    tile edges up to 6000, Hq / Hkv in {1, 2, 4}, full and banded, no / small / the handles' scratch, with and without a key-padding
    mask, MXFP8 output and a 128-CU hint."""
    import ctypes
    from ace355 import native
    lib = native.lib()
    rq, p = native.AttnRequestC(), native.AttnPlanInfoC()
    fn, rqp, pp = lib.ace355_attn_plan, ctypes.byref(rq), ctypes.byref(p)
    Sqs = sorted({e + d for e in (96, 128, 192, 256, 384, 1024, 1536) for d in (-1, 0, 1)} | {1, 20, 100, 125, 375, 750, 3000, 6000})
    Skvs = sorted({e + d for e in (64, 512, 1024) for d in (-1, 0, 1)} | {1, 375, 769, 1000, 6000})
    ATTN3, GQA, ROT = range(3)
    n, bad = 0, []
    for Hq, Hkv in ((2, 2), (2, 1), (4, 1), (16, 16), (16, 8), (16, 4)):
        for window in (-1, 16, 128):
            for part in (0, 1 << 20, cases.PART):
                for kvl, mx, cu in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 128), (1, 1, 128)):
                    rq.Hq, rq.Hkv, rq.window, rq.part_floats, rq.has_kv_len, rq.mx_out, rq.cu_slots = Hq, Hkv, window, part, kvl, mx, cu
                    for N in range(1, 17):
                        for Sq in Sqs:
                            for Skv in Skvs:
                                rq.N, rq.Sq, rq.Skv = N, Sq, Skv
                                assert fn(rqp, pp) == 0, native.last_error()
                                n += 1
                                rows = 32 * p.nw
                                why = None
                                if (p.kernel, p.nw) not in ((ATTN3, 4), (ATTN3, 8), (GQA, 3), (GQA, 4), (GQA, 6), (ROT, 3)):
                                    why = "one of the six instantiations"
                                elif p.kernel != ATTN3 and (p.grid_x % 8 or (p.grid_y, p.grid_z) != (1, 1) or p.grid_x < N * Hkv * -(-Sq // rows) or Hq != 2 * Hkv):
                                    why = "a 1-D grid, a multiple of 8, covering every (sequence, KV head, block), for Hq == 2 Hkv only"
                                elif p.kernel == ATTN3 and (p.grid_x, p.grid_y, p.grid_z, p.threads) != (-(-Sq // rows) * p.kv_split, Hq, N, 64 * p.nw):
                                    why = "attn3's grid is (blocks x parts, Hq, N)"
                                elif p.kernel != ATTN3 and p.threads != (768 if p.kernel == ROT else 128 * p.nw):
                                    why = "threads"
                                elif p.kv_split not in (1, 2, 4, 8):
                                    why = "kv_split in {1, 2, 4, 8}"
                                elif p.kv_split > 1 and not ((p.kernel, p.nw) == (ATTN3, 4) and part and not kvl and not mx and k_rotation != 0):
                                    why = "kv_split > 1 only for attn3<4> with scratch, no kv_len, no MX output and K rotation != 0"
                                elif p.kv_split * N * Hq * Sq * 132 > part and p.kv_split > 1:
                                    why = "the parts fit the scratch"
                                elif p.kernel == ROT and (k_rotation == 0 or mx):
                                    why = "rot never in the one-order mode or with MX output"
                                elif (p.merge_grid > 0) != (p.kv_split > 1) or (p.merge_grid and p.merge_grid != -(-N * Hq * Sq // 8)):
                                    why = "merge_grid > 0 iff kv_split > 1"
                                elif p.mx_out_ok != int(p.kernel != ATTN3 and not kvl):
                                    why = "mx_out_ok: a GQA-family kernel without a key-padding mask"
                                if why and len(bad) < 20:
                                    bad.append((why, dict(N=N, Sq=Sq, Skv=Skv, Hq=Hq, Hkv=Hkv, window=window, part=part, kvl=kvl, mx=mx, cu=cu),
                                                {f: getattr(p, f) for f, _t in native.AttnPlanInfoC._fields_}))
    print(f"{n} plans checked")
    for b in bad:
        print(b)
    assert not bad


def test_bad_requests_are_errors():
    from ace355 import native
    for rq in (dict(N=0, Sq=8, Skv=8, Hq=2, Hkv=1), dict(N=1, Sq=0, Skv=8, Hq=2, Hkv=1), dict(N=1, Sq=8, Skv=8, Hq=3, Hkv=2),
               dict(N=1, Sq=8, Skv=8, Hq=2, Hkv=0), dict(N=1, Sq=8, Skv=8, Hq=0, Hkv=1), dict(N=1, Sq=8, Skv=8, Hq=2, Hkv=1, part_floats=-1)):
        with pytest.raises(RuntimeError, match="attn_plan"):
            native.attn_plan(**rq)
