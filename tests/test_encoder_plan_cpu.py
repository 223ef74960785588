"""CPU: one pass of the encoder stack as data (csrc/encoder_plan.h, through ace355_encoder_pass_plan) - the launcher calls the cond, detok,
tok, textenc and lm handles make, in order.  A committed table pins request -> plan at full size and for the small configurations of the
GPU tests; the rows reach every step kind and both cached sub-paths; the closed-form call and FLOP counts hold; the decode steps carry
ace355_lm_decode_plan's cut; the refusals keep their texts; and a stand-alone program sweeps the invariants the executor and the allocator
rely on under the host sanitizers."""
import json
import os
import shutil
import subprocess

import pytest

import _encoder_plan_cases as cases


@pytest.fixture(scope="module")
def table():
    import ace355  # noqa: F401
    return json.load(open(cases.TABLE))


def test_plans_match_the_committed_table(table):
    """tests/encoder_plan_table.json, field by field.  A deliberate change of csrc/encoder_plan.h regenerates it
    (python tests/_encoder_plan_cases.py --write); its diff then shows which calls moved."""
    now = json.loads(json.dumps(cases.evaluate()))
    assert [r["name"] for r in table] == [r["name"] for r in now], "the table's rows are not the requests of tests/_encoder_plan_cases.py: regenerate it"
    bad = []
    for want, got in zip(table, now):
        assert (want["config"], want["N"], want["S"], want["fields"]) == (got["config"], got["N"], got["S"], got["fields"]), want["name"]
        w, g = want["plan"], got["plan"]
        bad += [f"{want['name']}: {k}: (got, table) {g.get(k)!r} {w.get(k)!r}" for k in sorted(set(w) | set(g)) if k != "steps" and w.get(k) != g.get(k)]
        assert len(w.get("steps", [])) == len(g.get("steps", [])), want["name"]
        for i, (ws, gs) in enumerate(zip(w.get("steps", []), g.get("steps", []))):
            bad += [f"{want['name']}: step {i} ({ws.get('kind')} layer {ws.get('layer')}).{k}: (got, table) {gs.get(k)!r} {ws.get(k)!r}"
                    for k in sorted(set(ws) | set(gs)) if ws.get(k) != gs.get(k)]
    print("\n".join(bad[:60]))
    assert not bad, f"{len(bad)} differences from the table"


def test_the_table_covers_what_it_claims(table):
    """Every step kind; the three paths; both cached sub-paths with left padding; key counts; a sliding layer next to a full one; a causal
    stack with more layers than the mask has bits."""
    from ace355 import native
    rows = {r["name"]: r for r in table}
    assert {k for r in table for k, n in r["plan"]["calls"].items() if n} == set(native.ENC_STEPS)
    cached = [r for r in table if r["fields"].get("has_cache")]
    assert any(r["fields"]["pos0"] == 0 and r["fields"]["has_first"] and r["plan"]["calls"]["causal_attn"] and r["plan"]["calls"]["kv_store"] for r in cached)
    assert any(r["fields"]["pos0"] > 0 and r["fields"]["has_first"] and r["plan"]["calls"]["decode_attn"] and r["plan"]["calls"]["kv_store"] for r in cached)
    assert any(r["fields"]["pos0"] + r["S"] == r["fields"]["max_pos"] for r in cached)
    assert any(r["plan"]["calls"]["vmean"] for r in table) and any(r["plan"]["calls"]["attn"] and not r["plan"]["calls"]["vmean"] for r in table)
    steps = rows["tiny: lyrics 2 x 70 with key counts, layer 0 sliding"]["plan"]["steps"]
    assert [s["kind"] for s in steps] == ["rmsnorm", "gemm", "transpose_v", "vmean", "attn", "gemm", "rmsnorm", "gemm", "gemm", "rmsnorm"]
    assert [s["window"] for s in steps if s["kind"] == "attn"] == [16] and steps[4]["kv_len"] == 1 and steps[4]["Sp"] == 128
    full = native.encoder_pass_plan(*cases.CONFIGS["tiny"], 2, 70, has_kv_len=1, sliding_window=16, sliding_layer_mask=1)
    assert [s["window"] for s in full["steps"] if s["kind"] == "attn"] == [16, -1]
    many = rows["tiny65: text 1 x 8, more layers than mask bits"]["plan"]
    assert many["calls"]["causal_attn"] == 65 and many["n_steps"] == 65 * 7 + 1
    # a prefill binds the first keys only where the cache has them; a pass without a cache never does
    assert {s["first"] for s in rows["tiny: LM prefill 3 x 17, left padding"]["plan"]["steps"] if s["kind"] == "causal_attn"} == {1}
    assert {s["first"] for s in rows["tiny: LM prefill without first keys"]["plan"]["steps"] if s["kind"] == "causal_attn"} == {0}
    assert {s["first"] for s in rows["tiny: text 2 x 65"]["plan"]["steps"] if s["kind"] == "causal_attn"} == {0}
    # the rope tables cover the cache, and a decode step's rows start at its position
    dec = rows["tiny: LM decode step at length 257, left padding"]["plan"]
    assert dec["rope_rows"] == 1100 and {s["rope_row0"] for s in dec["steps"] if s["kind"] == "gemm" and s["proj"] == "qkv"} == {256}
    assert {s["pos0"] for s in dec["steps"] if s["kind"] == "kv_store"} == {256}


def test_counts_are_the_closed_forms(table):
    """Launcher calls per layer for each path - two norms and four GEMMs everywhere, plus transpose_v (+ vmean) + attention, or (store +)
    causal attention, or store + decode attention - and the final norm; GEMM FLOPs 2 M N K over the four projections."""
    for r in table:
        D, F, HQ, KVH, NL = cases.CONFIGS[r["config"]]
        f, p = r["fields"], r["plan"]
        M, QD, QKV = r["N"] * r["S"], HQ * 128, (HQ + 2 * KVH) * 128
        causal, cached, decode = bool(f.get("causal")), bool(f.get("has_cache")), bool(f.get("has_cache")) and f["pos0"] > 0
        want = {"rmsnorm": 2 * NL + 1, "gemm": 4 * NL, "kv_store": NL * cached, "causal_attn": NL * (causal and not decode), "decode_attn": NL * decode,
                "transpose_v": NL * (not causal), "vmean": NL * (not causal and bool(f.get("has_kv_len"))), "attn": NL * (not causal)}
        assert p["calls"] == want and p["n_steps"] == sum(want.values()), r["name"]
        assert p["M"] == M and p["QKV"] == QKV and p["Sp"] == (r["S"] + 63) // 64 * 64 and p["rope_rows"] == (f["max_pos"] if cached else r["S"]), r["name"]
        assert p["gemm_flops"] == NL * (2 * M * QKV * D + 2 * M * D * QD + 2 * M * 2 * F * D + 2 * M * D * F), r["name"]


@pytest.mark.parametrize("length", [1, 2, 64, 65, 256, 257, 1024, 1025, 16384])
def test_decode_steps_carry_the_decode_plan(length):
    """Both sides of each regime boundary of csrc/lm_plan.h (256 | 257, 1024 | 1025): the decode steps of the pass plan at that length carry
    the chunk / splits ace355_lm_decode_plan gives for it."""
    from ace355 import native
    if length == 1:   # a cache of one key is a prefill of one column: no decode step
        p = native.encoder_pass_plan(*cases.CONFIGS["tiny"], 2, 1, **cases.cache(0, 16384, 2))
        assert p["calls"]["decode_attn"] == 0 and p["calls"]["causal_attn"] == 2
        return
    p = native.encoder_pass_plan(*cases.CONFIGS["tiny"], 2, 1, **cases.cache(length - 1, 16384, 2))
    d = native.lm_decode_plan(length)
    dec = [s for s in p["steps"] if s["kind"] == "decode_attn"]
    assert len(dec) == 2 and all((s["len"], s["chunk"], s["splits"]) == (length, d["chunk"], d["splits"]) for s in dec)
    assert d["chunk"] == (64 if length <= 256 else 128 if length <= 1024 else 256)


def test_refusals_keep_their_texts():
    from ace355 import native
    for text, kw in cases.REFUSALS:
        with pytest.raises(RuntimeError) as e:
            native.encoder_pass_plan(**{**cases.TINY, **kw})
        assert str(e.value).endswith("invalid argument: " + text), e.value
    for bad in (dict(N=0), dict(S=0), dict(num_kv_heads=0), dict(num_layers=257), dict(hidden_size=0)):
        with pytest.raises(RuntimeError, match="encoder_pass_plan"):
            native.encoder_pass_plan(**{**cases.TINY, "N": 1, "S": 4, **bad})


def test_sweep_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = tmp_path / "encoder_plan_sweep"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(cases.ROOT, "tests", "encoder_plan_sweep.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-3000:] + r.stderr[-4000:]
    print(r.stdout)
