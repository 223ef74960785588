"""CPU: the VAE's host side as data (csrc/vae_plan.h, through ace355_conv_plan / ace355_vae_plan) - which conv_kernel instantiation and
grid every conv launch of the project gets, and the step list a decode window / an encode group executes.  A committed table pins the
requests the product, the bench and the GPU tests make and four full step lists; fresh processes pin what each ACE355_CONV_* /
ACE355_VAE_* switch does to them; the step lists' data flow, the public stage lists, the buffer sizes and the window plans are checked
as properties; and a stand-alone program sweeps the stated conditions under the host sanitizers."""
import json
import os
import shutil
import subprocess
import sys

import pytest

import _vae_plan_cases as cases


@pytest.fixture(scope="module")
def table():
    import ace355  # noqa: F401
    return json.load(open(cases.TABLE))


def _diff(got, want):
    return {k: (got.get(k), want.get(k)) for k in sorted(set(got) | set(want)) if got.get(k) != want.get(k)}


def test_plans_match_the_committed_table(table):
    """tests/vae_plan_table.json, field by field.  A deliberate change of csrc/vae_plan.h regenerates it
    (python tests/_vae_plan_cases.py --write); its diff then shows which launches moved."""
    from ace355 import native
    now = cases.conv_rows()
    assert [r["name"] for r in table["conv"]] == [n for n, _r in now], "the table's rows are not the requests of tests/_vae_plan_cases.py: regenerate it"
    bad = []
    for row, (name, rq) in zip(table["conv"], now):
        if row["request"] != rq:
            bad.append(f"{name}: request {_diff(rq, row['request'])}")
        d = _diff(native.conv_plan(**rq), row["plan"])
        if d:
            bad.append(f"{name}: (got, table) {d}")
    assert [r["name"] for r in table["vae"]] == [r[0] for r in cases.VAE_ROWS]
    for row, (name, kw, enc, B, fr) in zip(table["vae"], cases.VAE_ROWS):
        got = cases.vae_call(kw, enc, B, fr)
        d = _diff({k: v for k, v in got.items() if k != "steps"}, {k: v for k, v in row["plan"].items() if k != "steps"})
        if d or len(got["steps"]) != len(row["plan"]["steps"]):
            bad.append(f"{name}: (got, table) {d}, {len(got['steps'])} / {len(row['plan']['steps'])} steps")
        for i, (g, w) in enumerate(zip(got["steps"], row["plan"]["steps"])):
            for k in sorted(set(g) | set(w)):
                if g.get(k) != w.get(k):
                    bad.append(f"{name}: step {i} {cases.step_name(w)}.{k}: (got, table) {g.get(k)!r} {w.get(k)!r}")
    print("\n".join(bad))
    assert not bad, f"{len(bad)} differences from the table"


def test_the_gpu_test_cases_are_on_the_forms_they_claim_and_reach_every_form(table):
    """The launch forms tests/test_vae_layers_gpu.py, test_fused_unit_forms_agree_bit_for_bit and test_conv1d_nlc name for their cases
    (tests/_vae_plan_cases.py) are the planned ones, and together the cases launch every instantiation plan_conv can emit."""
    from ace355 import native
    forms = set()
    for cid, kw, enc, B, fr, default, special in cases.LAYER_CASES:
        plan = cases.vae_call(kw, enc, B, fr)
        cases.assert_forms(plan, default, special, cid)
        assert all(k in {(st["weight"], st["Cin"]) for st in plan["steps"]} for k in special), f"{cid}: a claimed layer does not exist"
        forms |= {cases.form(st["plan"]) for st in plan["steps"]}
    for kw, enc, B, fr in cases.FUSED_FORM_CALLS:
        fused = [st for st in cases.vae_call(kw, enc, B, fr)["steps"] if st["fused"]]
        assert fused and all(cases.form(st["plan"]) == "w4" for st in fused)
    for row, want in cases.CONV1D_ROWS:
        p = native.conv_plan(**cases.conv1d_request(row))
        assert cases.form(p) == want, (row, p)
        forms.add(want)
    assert forms == cases.ALL_FORMS, forms
    # ... with and without rasterisation on each of the two forms that can carry it, full groups of 8 row blocks and the tail-only path
    ras = {(cases.form(r["plan"]), r["plan"]["ras_tn"] > 1, r["plan"]["ras_tm"] >= 8) for r in table["conv"] if r["name"].startswith("test_")}
    assert ras >= {("w4", True, True), ("w4", True, False), ("w4", False, False), ("w8", True, True), ("w8", True, False)}, ras


def test_public_stages_are_the_hand_written_list_of_old(table):
    """The stage lists read off the plan equal the library's former stage_list, restated as literals (tests/_vae_plan_cases.py)."""
    for name, kw, enc, B, fr in cases.VAE_ROWS:
        got = cases.stages_of(cases.vae_call(kw, enc, B, fr), enc)
        assert got == cases.EXPECTED_STAGES[name], [(i, g, w) for i, (g, w) in enumerate(zip(got, cases.EXPECTED_STAGES[name])) if g != w]


# ---------------------------------------------------------------------------------------------- switches: read once, so fresh processes
def _spawn(mode, env):
    cmd = [sys.executable, os.path.join(cases.ROOT, "tests", "_vae_plan_cases.py"), mode]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("ACE355_")}
    return subprocess.Popen(cmd, env={**clean, **env}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _gather(mode, envs):
    out = {}
    for i in range(0, len(envs), 6):   # six processes at a time
        procs = [(e, _spawn(mode, e)) for e in envs[i:i + 6]]
        for e, p in procs:
            so, se = p.communicate(timeout=600)
            assert p.returncode == 0, (e, se[-3000:])
            out[tuple(sorted(e.items()))] = json.loads(so)
    return out


EPI0, FUSE0 = {"ACE355_VAE_EPISNAKE": "0"}, {"ACE355_CONV_FUSE_RU": "0"}
KNOB_ENVS = [{"ACE355_CONV_RAS": "0"}, {"ACE355_CONV_TM": "128"}, {"ACE355_CONV_TM": "256"}, {"ACE355_CONV_F8": "0"}, {"ACE355_CONV_F8": "1"},
             FUSE0, EPI0, {"ACE355_CONV_CLK": "1"}, {**EPI0, **FUSE0}]


@pytest.fixture(scope="module")
def knob_plans():
    return _gather("--plans", KNOB_ENVS)


def _conv(knob_plans, table, **env):
    """(request, default plan, this setting's plan) of every conv row"""
    rows = knob_plans[tuple(sorted(env.items()))]["conv"]
    assert [r["name"] for r in rows] == [r["name"] for r in table["conv"]]
    return [(t["request"], t["plan"], r["plan"]) for t, r in zip(table["conv"], rows)]


def _only(d, p, *fields):
    """p differs from d in `fields` at most"""
    return all(p[k] == d[k] for k in d if k not in fields)


GRID = ("grid_x", "grid_y", "ras_tm", "ras_tn")


def test_knob_ras(knob_plans, table):
    rows = _conv(knob_plans, table, ACE355_CONV_RAS="0")
    assert any(d["ras_tn"] for _rq, d, _p in rows)
    for rq, d, p in rows:
        assert _only(d, p, *GRID) and p["ras_tm"] == p["ras_tn"] == 0, (rq, p)
        assert (p["grid_x"], p["grid_y"]) == ((d["ras_tm"], d["ras_tn"]) if d["ras_tn"] else (d["grid_x"], d["grid_y"])), (rq, p)


def test_knob_tm(knob_plans, table):
    rows = _conv(knob_plans, table, ACE355_CONV_TM="128")
    assert any(cases.form(d) == "w8" for _rq, d, _p in rows)
    for rq, d, p in rows:   # the plain tall tile goes; the fused 8-wave form and the 32-column tile are not a tile height
        assert (_only(d, p, "tm", "threads", *GRID) and cases.form(p) == "w4" and -(-rq["M"] // 128) in (p["grid_x"], p["ras_tm"])) if cases.form(d) == "w8" else p == d, (rq, p)
    rows = _conv(knob_plans, table, ACE355_CONV_TM="256")
    assert any(rq["res"] and d["bn"] == 128 for rq, d, _p in rows) and any(rq["fused"] for rq, _d, _p in rows)
    for rq, d, p in rows:   # never with w2 or a residual, also when forced
        if rq["fused"] or rq["res"] or d["bn"] == 32:
            assert p == d, (rq, p)
        else:
            assert _only(d, p, "tm", "threads", *GRID) and cases.form(p) == "w8" and -(-rq["M"] // 256) in (p["grid_x"], p["ras_tm"]), (rq, p)


def test_knob_f8(knob_plans, table):
    for v in ("0", "1"):
        rows = _conv(knob_plans, table, ACE355_CONV_F8=v)
        assert {cases.form(d) for rq, d, _p in rows if rq["fused"]} == {"w4", "f8"}
        for rq, d, p in rows:
            if not rq["fused"]:
                assert p == d, (rq, p)
            else:
                assert cases.form(p) == ("f8" if v == "1" else "w4") and p["ras_tn"] == 0 and p["grid_y"] == 1, (rq, p)
                assert p["grid_x"] == -(-rq["M"] // p["tm"]) and p["grid_z"] == rq["B"] and p["threads"] == 2 * p["tm"], (rq, p)
    # test_fused_unit_forms_agree_bit_for_bit's calls under F8=1: its one-launch units are on the 8-wave form there
    steps = knob_plans[(("ACE355_CONV_F8", "1"),)]["vae"]
    assert all(cases.form(st["plan"]) == "f8" for row in steps for st in row["plan"]["steps"] if st["fused"])


def test_knobs_outside_the_conv_plan(knob_plans, table):
    """CLK is a kernel argument; FUSE_RU and EPISNAKE change which requests a walk makes, not what a request gets."""
    for env in ({"ACE355_CONV_CLK": "1"}, FUSE0, EPI0, {**EPI0, **FUSE0}):
        assert all(p == d for _rq, d, p in _conv(knob_plans, table, **env)), env
    clk = knob_plans[(("ACE355_CONV_CLK", "1"),)]["vae"]
    assert [r["plan"] for r in clk] == [r["plan"] for r in table["vae"]]


SNAKE_FIELDS = ("in_snake", "in_snake_block", "out_snake", "out_snake_block", "stage_info", "plan")


def test_knobs_fuse_ru_and_episnake_on_the_step_lists(knob_plans, table):
    for env in (FUSE0, EPI0, {**EPI0, **FUSE0}):
        fuse0, epi0 = "ACE355_CONV_FUSE_RU" in env, "ACE355_VAE_EPISNAKE" in env
        for trow, row in zip(table["vae"], knob_plans[tuple(sorted(env.items()))]["vae"]):
            d, p = trow["plan"]["steps"], row["plan"]["steps"]
            assert any(st["fused"] for st in d)
            it = iter(p)
            for ds in d:   # the default list step by step; a fused unit becomes its two convs under FUSE_RU=0, nothing else moves
                ps = next(it)
                if ds["fused"] and fuse0:
                    k1 = next(it)
                    assert (ps["weight"], k1["weight"], ps["fused"], k1["fused"]) == ("unit_c1", "unit_c2", 0, 0)
                    assert ps["res"] is None and ps["dst"] != ps["src"] and (k1["src"], k1["dst"], k1["res"]) == (ps["dst"], ps["src"], ps["src"])
                    assert all(ps[k] == ds[k] == k1[k] for k in ("block", "unit", "Cin", "N", "M", "L_in", "y_valid"))
                    assert (ps["taps"], ps["dil"], k1["taps"], k1["dil"]) == (7, ds["dil"], 1, 1)
                    assert k1["out_snake"] == (None if epi0 else ds["out_snake"])
                    continue
                # (after a split unit the state stays in its slot instead of trading places: slot names may differ from the default's)
                same = [k for k in ds if k not in SNAKE_FIELDS + (("src", "dst", "res", "stage") if fuse0 else ())]
                assert all(ps[k] == ds[k] for k in same), (env, cases.step_name(ds), {k: (ps[k], ds[k]) for k in same if ps[k] != ds[k]})
                if not epi0:
                    assert all(ps[k] == ds[k] for k in SNAKE_FIELDS[:4])
            assert next(it, None) is None
            assert not fuse0 or not any(st["fused"] for st in p)
            if epi0:   # every Snake in its reader's staging: no producer applies one, every reader but the first conv does
                assert not any(st["out_snake"] for st in p)
                assert all((st["in_snake"] is None) == (st["weight"] == "conv_in") for st in p)


def test_step_list_properties_under_the_four_snake_and_fusion_settings():
    """tests/_vae_plan_cases.py check_properties over SMALL, the default, a one-block and an odd-hop configuration, both halves, 1 frame
    to lengths that are a multiple of nothing - in a process per (EPISNAKE, FUSE_RU) setting."""
    got = _gather("--properties", [{}, EPI0, FUSE0, {**EPI0, **FUSE0}])
    assert len(got) == 4 and all(v["checked"] == 4 * len(cases.PROPERTY_LENGTHS) * 2 * 3 for v in got.values()), got


# ---------------------------------------------------------------------------------------------- sizes and windows
def _parent_decode_elems(cfg, frames):
    """What the decoder allocated before the sizes were read off the plan: the largest stage, L * C (restated once, here)."""
    dims, need, L = cfg.block_dims(), frames * cfg.block_dims()[0][0], frames
    for _cin, cout, s in dims:
        L = (L - 1) * s - 2 * ((s + 1) // 2) + 2 * s
        need = max(need, L * cout)
    return need


def test_buffer_sizes_equal_the_former_formulas_and_cover_a_growing_encoder():
    """slot_elems is a maximum over the plan's steps.  For every configuration of the table it equals what the library allocated before:
    the decoder's maximum over stages, the encoder's first stage (items x samples x encoder width).  The encoder formula ASSUMED the first
    stage is the largest; with channel multiples that grow faster than the stride shrinks the length a later stage is larger, and the
    former formula under-allocated there: the plan's size covers it."""
    import ace355
    from ace355 import native
    for kw in (cases.SMALL, cases.FULL):
        cfg = ace355.VaeConfig(**kw)
        for frames in (1, 9, 24, 37, 280, 750, 3000):
            assert native.vae_plan(cfg, False, 1, frames)["slot_elems"] == _parent_decode_elems(cfg, frames), (kw, frames)
            L = cfg.hop * frames
            assert native.vae_plan(cfg, True, 1, L)["slot_elems"] == L * 2 * cfg.decoder_input_channels, (kw, frames)
    grow = ace355.VaeConfig(decoder_channels=64, channel_multiples=(4,), downsampling_ratios=(2,))
    L = 4096
    p = native.vae_plan(grow, True, 1, L)
    down = [st for st in p["steps"] if st["weight"] == "down"][0]
    assert down["y_valid"] == (L // 2) * 4 * 128 == 2 * L * 128 and p["slot_elems"] == down["y_valid"] > L * 128


def test_window_plans():
    """Under a budget: the first window starts at frame 0 with one halo, cores are whole 8-frame groups unless whole, the halo covers the
    receptive field (restated here), the bytes stay within the budget (to the buffers' tails), and the step list is that window's."""
    import math
    import ace355
    from ace355 import native
    for kw in (cases.SMALL, cases.FULL, cases.ONE_BLOCK):
        cfg = ace355.VaeConfig(**kw)
        rf, rate = 3.0, 1.0
        for s in cfg.upsampling_ratios:
            rf += 1.0 / rate
            rate *= s
            rf += 39.0 / rate
        rf = math.ceil(rf + 3.0 / rate)
        for B, T in ((1, 200), (3, 200), (2, 750)):
            whole = native.vae_plan(cfg, False, B, T)
            assert (whole["items_per_window"], whole["core_frames"], whole["window_len"]) == (B, T, T) and whole["overlap_frames"] >= max(rf, 16)
            for div in (2, 3, 4, 8, 16):
                budget = whole["activation_bytes"] // div
                try:
                    p = native.vae_plan(cfg, False, B, T, budget_bytes=budget)
                except RuntimeError as e:   # smaller than one window with its two halos: refused, never at the 30 s length
                    assert "budget is smaller than one decode window" in str(e) and T < 750 and div > 2, (kw, B, T, div, e)
                    continue
                nb, tc, ov = p["items_per_window"], p["core_frames"], p["overlap_frames"]
                # within the budget - up to the three buffers' 256-byte tails: the window length comes from bytes per frame measured on a
                # 1024-frame window, tails included, so a shorter window's estimate lacks up to 768 bytes of them (and never more: the
                # stage lengths are s L - c, c >= 0, so elements per frame do not fall with the length).  DESIGN 21.
                assert p["activation_bytes"] < budget + 768 and 1 <= nb <= B and ov >= rf and (nb < B or tc < T), (kw, B, T, div, p["activation_bytes"])
                assert tc == T or (tc % 8 == 0 and 0 < tc < T and p["window_len"] == min(T, tc + ov)), (tc, p["window_len"])
                out = p["steps"][-1]
                assert (out["ncl_off"], out["ncl_m_lo"], out["ncl_m_hi"], out["ncl_ld"]) == (0, 0, min(tc, T) * cfg.hop, T * cfg.hop)
                assert p["steps"][0]["x_batch_stride"] == T * 64 and p["steps"][0]["M"] == p["window_len"]
            if T == 750:
                assert native.vae_plan(cfg, False, B, T, budget_bytes=whole["activation_bytes"] // 2, overlap_frames=64)["overlap_frames"] == 64
        with pytest.raises(RuntimeError, match="receptive field"):
            native.vae_plan(cfg, False, 1, 100, overlap_frames=1)
        with pytest.raises(RuntimeError, match="budget"):
            native.vae_plan(cfg, False, 1, 100, budget_bytes=4096)
    full = ace355.VaeConfig()
    for n in (1, 12, 750):
        assert native.vae_plan(full, True, 1, full.hop * n)["out_len"] == n
    # (C++ division truncates towards zero, so floor((L + 2 pad - 2 s) / s) + 1 never falls below 1 for L >= 1: the "shorter than one
    #  latent frame" refusal of the encoder cannot fire for a positive length.  Kept as it was.)
    assert native.vae_plan(full, True, 1, 3)["out_len"] == 1


def test_invariants_over_a_sweep_through_the_hook():
    """What vae_plan.h states about a conv plan, through ace355_conv_plan: B 1 / 2 / 8, M around every multiple of 256 up to 4300 and the
    metric lengths, every width, taps and bit.  (The full grid - B 1 .. 8, every multiple of 128, every switch setting - runs in
    tests/vae_plan_sweep.cpp, where a call costs nanoseconds.)"""
    import ctypes
    from ace355 import native
    lib = native.lib()
    rq, p = native.ConvRequestC(), native.ConvPlanInfoC()
    fn, rqp, pp = lib.ace355_conv_plan, ctypes.byref(rq), ctypes.byref(p)
    Ms = sorted({e + d for e in range(256, 4301, 256) for d in (-1, 0, 1)} | {1, 127, 129, 750, 45000, 1440000})
    n, bad = 0, []
    for N in (2, 64, 128, 256, 512, 1024, 2048, 1280, 3072, 10240):
        for Cin in (64, 128, 512, 2048):
            for taps in (1, 2, 3, 7):
                for bits in range(16):
                    rq.N, rq.Cin, rq.taps, rq.in_snake, rq.x_view, rq.res, rq.fused = N, Cin, taps, bits & 1, (bits >> 1) & 1, (bits >> 2) & 1, bits >> 3
                    if rq.fused and not (Cin == 128 and N == 128 and taps == 7 and not rq.x_view):
                        continue
                    for B in (1, 2, 8):
                        for M in Ms:
                            rq.B, rq.M = B, M
                            assert fn(rqp, pp) == 0, native.last_error()
                            n += 1
                            tn = 1 if p.ws else -(-N // p.bn)
                            why = None
                            if (p.bn, p.tm, p.ws) not in cases.FORMS or (p.bn == 32) != (N < 128):
                                why = "one of the four instantiations; the 32-column tile iff N < 128"
                            elif p.threads != 2 * p.tm or p.grid_z != B:
                                why = "threads = 2 tm, one grid plane per item"
                            elif (p.ras_tn > 1) != (tn > 1 and p.bn == 128) or (p.ras_tn and (p.ras_tm, p.ras_tn, p.grid_x, p.grid_y) != (-(-M // p.tm), tn, -(-M // p.tm) * tn, 1)):
                                why = "rasterised iff more than one column tile, never with ws = 1"
                            elif not p.ras_tn and (p.grid_x, p.grid_y, p.ras_tm) != (-(-M // p.tm), tn, 0):
                                why = "the grid covers M x N"
                            elif p.ws and not rq.fused:
                                why = "ws = 1 only with fused"
                            elif (rq.fused or rq.res) and p.tm == 256 and not p.ws:
                                why = "fused / res never tall"
                            if why and len(bad) < 20:
                                bad.append((why, {f: getattr(rq, f) for f, _t in native.ConvRequestC._fields_}, {f: getattr(p, f) for f, _t in native.ConvPlanInfoC._fields_}))
    print(f"{n} plans checked")
    for b in bad:
        print(b)
    assert not bad


def test_bad_requests_are_errors():
    import ace355
    from ace355 import native
    for rq in (dict(B=0, M=8, N=8, Cin=64, taps=1), dict(B=1, M=0, N=8, Cin=64, taps=1), dict(B=1, M=8, N=8, Cin=32, taps=1),
               dict(B=1, M=8, N=8, Cin=64, taps=0), dict(B=1, M=8, N=256, Cin=256, taps=7, fused=1)):
        with pytest.raises(RuntimeError, match="conv_plan"):
            native.conv_plan(**rq)
    with pytest.raises(RuntimeError, match="channels"):
        native.vae_plan(ace355.VaeConfig(decoder_channels=96), False, 1, 8)
    with pytest.raises(RuntimeError, match="vae_plan"):
        native.vae_plan(ace355.VaeConfig(), False, 0, 8)


# ---------------------------------------------------------------------------------------------- the stand-alone program
def _sweep_input(path, table):
    import ace355
    with open(path, "w") as f:
        for r in table["conv"]:
            rq, p = r["request"], r["plan"]
            f.write("C " + " ".join(str(rq[k]) for k in ("B", "M", "N", "Cin", "taps", "in_snake", "x_view", "res", "fused")) + " " +
                    " ".join(str(p[k]) for k in ("bn", "tm", "ws", "grid_x", "grid_y", "grid_z", "threads", "ras_tm", "ras_tn")) + "\n")
        for name, kw, enc, B, fr in cases.calls():
            cfg = ace355.VaeConfig(**kw)
            p = cases.vae_call(kw, enc, B, fr)
            cm, ups = list(cfg.channel_multiples), list(cfg.upsampling_ratios)
            f.write(f"V {cfg.decoder_channels} {cfg.decoder_input_channels} {cfg.audio_channels} {len(cm)} " + " ".join(map(str, cm + ups)) +
                    f" {int(enc)} {B} {fr * cfg.hop if enc else fr} {p['n_steps']} {p['slot_elems']}\n")


def test_sweep_under_host_sanitizers(tmp_path, table):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe, inp = tmp_path / "vae_plan_sweep", tmp_path / "calls.txt"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(cases.ROOT, "tests", "vae_plan_sweep.cpp"), "-o", str(exe)], check=True)
    _sweep_input(inp, table)
    r = subprocess.run([str(exe), str(inp), "1500"], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    print(r.stdout)
    n = len(table["conv"]) + len(cases.calls())
    assert f"{n} listed rows as expected" in r.stdout and "1500 random calls" in r.stdout
