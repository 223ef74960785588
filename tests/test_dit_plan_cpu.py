"""CPU: one decoder pass as data (csrc/dit_plan.h, through ace355_dit_pass_plan) - the launches a handle makes for a forward, a sampler
step or a maps call, in order.  A committed table pins request -> plan at full size and for the two small configurations of the GPU tests;
fresh processes pin what each process switch does to it; the refusals keep forward's texts; the closed-form launch and FLOP counts hold;
and a stand-alone program sweeps the invariants the executor relies on under the host sanitizers."""
import json
import os
import shutil
import subprocess
import sys

import pytest

import _dit_plan_cases as cases


@pytest.fixture(scope="module")
def table():
    import ace355  # noqa: F401
    return json.load(open(cases.TABLE))


def test_plans_match_the_committed_table(table):
    """tests/dit_plan_table.json, field by field.  A deliberate change of csrc/dit_plan.h regenerates it
    (python tests/_dit_plan_cases.py --write); its diff then shows which launches moved."""
    now = cases.evaluate()
    assert [r["name"] for r in table] == [r["name"] for r in now], "the table's rows are not the requests of tests/_dit_plan_cases.py: regenerate it"
    bad = []
    for want, got in zip(table, json.loads(json.dumps(now))):
        assert (want["config"], want["T"], want["seqs"], want["fields"]) == (got["config"], got["T"], got["seqs"], got["fields"]), want["name"]
        w, g = want["plan"], got["plan"]
        bad += [f"{want['name']}: {k}: (got, table) {g.get(k)!r} {w.get(k)!r}" for k in sorted(set(w) | set(g)) if k != "steps" and w.get(k) != g.get(k)]
        for i, (ws, gs) in enumerate(zip(w.get("steps", []), g.get("steps", []))):
            bad += [f"{want['name']}: step {i} ({ws.get('kind')} {ws.get('proj', '')} layer {ws.get('layer', -1)}).{k}: (got, table) {gs.get(k)!r} {ws.get(k)!r}"
                    for k in sorted(set(ws) | set(gs)) if ws.get(k) != gs.get(k)]
    print("\n".join(bad[:60]))
    assert not bad, f"{len(bad)} differences from the table"


def test_the_table_covers_what_it_claims(table):
    """The rows reach every step kind, every GEMM path, both attention kinds with and without MXFP8 output, the shortcut, the generic path,
    the deduplicated layer 0, the early exit of a maps call, and both memset answers."""
    rows = {r["name"]: r["plan"] for r in table}
    steps = [s for p in rows.values() for s in p.get("steps", [])]
    kinds = set().union(*(p["kinds"] for p in rows.values()))   # over ALL steps of every row: "kind", GEMMs as "gemm:path"
    from ace355 import native
    assert {k.split(":")[0] for k in kinds} == set(native.DIT_STEPS) - {"norm_w_mx"}   # (the cross-attention MX norm: ACE355_MX_CROSS=1, below)
    assert {k.split(":")[1] for k in kinds if ":" in k} == set(native.DIT_PATHS)
    assert {(s["kind"], s.get("mx_out", 0)) for s in steps if s["kind"].startswith("attn")} == {("attn_self", 0), ("attn_self", 1), ("attn_cross", 0)}
    assert rows["full: 1 songs, CFG, sampler (folded norms)"]["dedup0"] == 1 and rows["full: dedup off"]["dedup0"] == 0 and rows["full: layers 0 and 1 tapped"]["dedup0"] == 0
    assert rows["full: null slot not broadcast (the generic path)"]["n_sc"] == 0 and rows["full: two broadcast slots at the end (no shortcut)"]["n_sc"] == 0
    assert rows["full: cover switch onto slots of another L (the null slot keeps the cover phase's)"]["L"] == 809
    assert rows["full: zero row in place"]["zero_rows"] == 0 and rows["full: graph mode, zero row in place"]["zero_rows"] == 1
    assert rows["full: maps stopping at a middle layer"]["gemm_launches"] == 1 + 6 * 12 + 3
    assert rows["tiny: maps stopping at a middle layer"]["steps"][-1]["kind"] == "xattn_probs"
    # a mid-size MXFP8 pass quantises its bf16 operands (D != 2048: no norm writes MXFP8), the full-size one gets them from the producers
    mid = rows["mid: metric batch, MXFP8"]["steps"]
    assert {(s["proj"], s["path"]) for s in mid if s["kind"] == "gemm" and s.get("layer", -1) >= 0} == {
        ("qkv", "mx_quant"), ("o", "mx"), ("cross_q", "bf16"), ("cross_o", "bf16"), ("gate_up", "mx_quant"), ("down", "mx_quant")}   # (o: from the attention epilogue)
    assert "norm_gs_mx" not in {s["kind"] for s in mid}
    assert "gemm:mx_quant" not in rows["full: metric batch, MXFP8"]["kinds"]


def test_counts_are_the_closed_forms(table):
    """GEMM launches: patchify + 6 per layer (4 without conditional rows) + proj_out; GEMM FLOPs: 2 M N K over them, with layer 0's QKV on
    the conditional half where the step is deduplicated."""
    for r in table:
        cfg, p = cases.config(r["config"]), r["plan"]
        if r["fields"].get("map_last", -1) >= 0:
            continue
        nl, D, F = cfg.num_hidden_layers, cfg.hidden_size, cfg.intermediate_size
        QD, KVD = cfg.num_attention_heads * 128, cfg.num_key_value_heads * 128
        M, Mc = p["M"], p["Mc"]
        assert p["gemm_launches"] == 1 + 6 * nl + 1, r["name"]
        per_layer = 2 * M * (QD + 2 * KVD) * D + 2 * M * D * QD + 2 * Mc * QD * D + 2 * Mc * D * QD + 2 * M * 2 * F * D + 2 * M * D * F
        want = 2 * M * D * 2 * cfg.in_channels + nl * per_layer + 2 * M * 128 * D - (2 * (M - Mc) * (QD + 2 * KVD) * D if p["dedup0"] else 0)
        assert p["gemm_flops"] == want, r["name"]


def test_refusals_keep_forwards_texts():
    from ace355 import native
    cfg = cases.config("tiny")
    for text, seqs in cases.REFUSALS:
        with pytest.raises(RuntimeError) as e:
            native.dit_pass_plan(cfg, 37, seqs)
        assert str(e.value).endswith("invalid argument: " + text), e.value
    # the slot check comes first, as in forward
    with pytest.raises(RuntimeError, match="condition slot not set"):
        native.dit_pass_plan(cfg, 37, [(0, 5, 0), (1, 6, 0), (2, 0, 0)])
    for bad in (dict(T=0), dict(seqs=[]), dict(temb_rows=3), dict(map_last=5, map_heads=[1, 1]), dict(map_last=1, map_heads=[1, 0])):
        kw = {"T": 37, "seqs": [(0, 5, 0), (1, 5, 0)], **bad}
        with pytest.raises(RuntimeError, match="dit_pass_plan"):
            native.dit_pass_plan(cfg, kw.pop("T"), kw.pop("seqs"), **kw)


# ---------------------------------------------------------------------------------------------- switches: read once, so fresh processes
KNOB_ENVS = [{"ACE355_GEMM_ZROW": "0"}, {"ACE355_MX_MASK": "61"}, {"ACE355_MX_CROSS": "1"}, {"ACE355_SCHED_TABLES": "0"}]


@pytest.fixture(scope="module")
def knob_plans():
    clean = {k: v for k, v in os.environ.items() if not k.startswith("ACE355_")}
    procs = [(e, subprocess.Popen([sys.executable, os.path.join(cases.ROOT, "tests", "_dit_plan_cases.py"), "--plans"], env={**clean, **e},
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)) for e in KNOB_ENVS]
    out = {}
    for e, p in procs:
        so, se = p.communicate(timeout=600)
        assert p.returncode == 0, (e, se[-3000:])
        out[next(iter(e))] = {r["name"]: r["plan"] for r in json.loads(so)}
    return out


def _same_but(a, b, *fields):
    return {k: v for k, v in a.items() if k not in fields} == {k: v for k, v in b.items() if k not in fields}


def test_zero_row_switch(table, knob_plans):
    """ACE355_GEMM_ZROW=0: no launch names a zero row and no call zeroes one; nothing else moves."""
    for r in table:
        d, k = r["plan"], knob_plans["ACE355_GEMM_ZROW"][r["name"]]
        assert k["zero_rows"] == 0 and k["sha256"] != d["sha256"] and _same_but(d, k, "zero_rows", "steps", "sha256"), r["name"]
        if "steps" not in d:
            continue
        assert len(d["steps"]) == len(k["steps"])
        for sd, sk in zip(d["steps"], k["steps"]):
            assert "a_zero_idx" not in sk and _same_but(sd, sk, "a_zero_idx"), r["name"]
        assert any("a_zero_idx" in s for s in d["steps"])


def test_mx_switches(table, knob_plans):
    """ACE355_MX_MASK=61 keeps o_proj in bf16 (and its attention output with it); ACE355_MX_CROSS=1 moves the cross-attention q / o
    projections of the full-size MXFP8 rows onto the MX path, fed by the MXFP8 norm and, where the kernel can, the attention epilogue.
    Neither touches a bf16 row."""
    for r in table:
        d = r["plan"]
        for env in ("ACE355_MX_MASK", "ACE355_MX_CROSS"):
            k = knob_plans[env][r["name"]]
            if r["fields"].get("precision", 0) != 1 or d["M"] < 1536:
                assert k == d, (env, r["name"])
    name = "full: metric batch, MXFP8"
    d, m, c = next(r["plan"] for r in table if r["name"] == name), knob_plans["ACE355_MX_MASK"][name], knob_plans["ACE355_MX_CROSS"][name]
    path = lambda p, proj: {s["path"] for s in p["steps"] if s["kind"] == "gemm" and s["proj"] == proj}
    assert path(d, "o") == {"mx"} and path(m, "o") == {"bf16"} and all(s.get("mx_out", 0) == 0 for s in m["steps"] if s["kind"] == "attn_self")
    assert path(m, "qkv") == path(d, "qkv") == {"mx"} and path(m, "down") == path(d, "down") == {"mx"}
    assert path(d, "cross_q") == path(d, "cross_o") == {"bf16"} and path(c, "cross_q") == {"mx"} and path(c, "cross_o") <= {"mx", "mx_quant"}
    assert "norm_w_mx" in {s["kind"] for s in c["steps"]} and "norm_w" not in {s["kind"] for s in c["steps"]}


def test_sched_tables_switch_leaves_the_pass_alone(table, knob_plans):
    """ACE355_SCHED_TABLES acts where a sampler call prepares its tables (the request's nf_on / nf_emb_on), not in the pass."""
    assert all(knob_plans["ACE355_SCHED_TABLES"][r["name"]] == r["plan"] for r in table)


# ---------------------------------------------------------------------------------------------- the stand-alone program
def test_sweep_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = tmp_path / "dit_plan_sweep"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(cases.ROOT, "tests", "dit_plan_sweep.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), "6000"], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-3000:] + r.stderr[-4000:]
    print(r.stdout)
