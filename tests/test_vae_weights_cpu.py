"""CPU: the weights of a VAE handle as data (vae_weight_table of csrc/vae_plan.h) - one row per conv and per Snake, which
ace355_vae_finalize walks, a step's role resolves to, and config.py's weight_shapes() / encoder_weight_shapes() restate.  A stand-alone
program (tests/vae_weights_sweep.cpp), built under the host sanitizers, checks the pack index of every layout against the formulas the
four former pack kernels held and prints the table; here the table is held against config.py and against the steps of plan_vae."""
import json
import math
import os
import shutil
import subprocess

import pytest

import _vae_plan_cases as cases

ONE_BLOCK = dict(decoder_channels=64, channel_multiples=(2,), downsampling_ratios=(4,))
MONO = dict(audio_channels=1)
CONFIGS = {"default": cases.FULL, "small": cases.SMALL, "one-block": ONE_BLOCK, "mono": MONO}
SNAKE = 4   # VAE_ROW_SNAKE


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """The program, built once: -Wall -Wextra -Werror, AddressSanitizer and UBSan, its own process, no LD_PRELOAD."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = tmp_path_factory.mktemp("vae_weights") / "vae_weights_sweep"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(cases.ROOT, "tests", "vae_weights_sweep.cpp"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def tables(sweep):
    """name -> the table of both halves; each run also sweeps the pack index and must end with status 0 and an empty stderr."""
    out = {}
    for name, kw in CONFIGS.items():
        cfg = cases.vae_config(kw)
        args = [cfg.decoder_channels, cfg.decoder_input_channels, cfg.audio_channels, len(cfg.channel_multiples), *cfg.channel_multiples,
                *cfg.upsampling_ratios]
        r = subprocess.run([sweep, *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, (name, r.stdout[-2000:] + r.stderr[-4000:])
        out[name] = json.loads(r.stdout)
    return out


def test_pack_index_and_slots_under_host_sanitizers(tables):
    """The program's own checks passed for every configuration (the fixture asserts status and stderr): vae_pack_index is injective into
    the packed weight, onto except for im2col's zero columns, equal to the four former formulas, the norm's rows and columns and the packed
    (N, taps, Cin) are the former builders', and every row sits at vae_weight_slot of its role."""
    assert set(tables) == set(CONFIGS)
    for t in tables.values():
        assert len(t["decoder"]) == len(t["encoder"]) > 0


@pytest.mark.parametrize("name", list(CONFIGS))
def test_table_lists_the_tensors_of_config_py(tables, name):
    cfg = cases.vae_config(CONFIGS[name])
    for half, shapes in (("decoder", cfg.weight_shapes()), ("encoder", cfg.encoder_weight_shapes())):
        rows = tables[name][half]
        listed = [kv for r in rows for kv in r["tensors"].items()]
        assert len(listed) == len(dict(listed)), "a tensor named by two rows"
        assert dict(listed) == {k: math.prod(v) for k, v in shapes.items()}, half
        # the pre-fused form: base.weight with weight_v's size in place of the pair, nothing else moves
        for r in rows:
            want = {k.replace(".weight_v", ".weight"): n for k, n in r["tensors"].items() if not k.endswith(".weight_g")}
            assert r["tensors_fused"] == want, r["base"]
        # state-dict order of the bases
        bases = list(dict.fromkeys(k.rsplit(".", 1)[0] for k in shapes))
        assert [r["base"] for r in rows] == bases, half
        for r in rows:
            if r["kind"] == SNAKE:
                # repeated `stride` times for an encoder block's own Snake (the strided conv's virtual channels), once otherwise
                own = half == "encoder" and r["base"].count(".") == 3
                assert r["s"] == (cfg.downsampling_ratios[r["block"]] if own else 1), r["base"]


def _resolve(rows, snake, name, block, unit):
    """The rows a step's role names: FINAL / CONV_IN / OUT / HEAD by role alone, a block's own Snake and conv by block, a unit's by both."""
    from ace355 import native
    idx = (native.VAE_SNAKES if snake else native.VAE_WEIGHTS).index(name)
    by_block, by_unit = name in ("unit_s1", "unit_s2", "block", "convt", "unit_c1", "unit_c2", "down"), name.startswith("unit_")
    return [i for i, r in enumerate(rows) if (r["kind"] == SNAKE) == snake and r["role"] == idx and (not by_block or r["block"] == block)
            and (not by_unit or r["unit"] == unit)]


@pytest.mark.parametrize("name", ["default", "small"])
@pytest.mark.parametrize("enc", [False, True])
def test_steps_and_rows_correspond(tables, name, enc):
    """Every weight and Snake a step of plan_vae names is exactly one row, whose packed (N, taps, Cin) are the step's; a fused step's second
    stage is the unit's snake2 and conv2, as run_plan (csrc/vae.hip) reads it; and no row is left unnamed."""
    rows = tables[name]["encoder" if enc else "decoder"]
    plan = cases.vae_call(CONFIGS[name], enc, 1, 8)
    used = set()
    for st in plan["steps"]:
        got = _resolve(rows, False, st["weight"], st["block"], st["unit"])
        assert len(got) == 1, (cases.step_name(st), got)
        w = rows[got[0]]
        assert (w["N"], w["taps"], w["Cin"]) == (st["N"], st["taps"], st["Cin"]), (cases.step_name(st), w)
        used.add(got[0])
        for which in ("in_snake", "out_snake"):
            if st[which] is not None:
                got = _resolve(rows, True, st[which], st[which + "_block"], st["unit"])
                assert len(got) == 1, (cases.step_name(st), which, got)
                sn = rows[got[0]]
                # a Snake on the input covers the step's input channels (the strided conv's: the pair repeated over its virtual channels),
                # one in the epilogue the output channels
                assert (sn["d0"] * sn["s"] == st["Cin"]) if which == "in_snake" else (sn["d0"] == st["N"]), (cases.step_name(st), which, sn)
                used.add(got[0])
        if st["fused"]:
            c2, s2 = _resolve(rows, False, "unit_c2", st["block"], st["unit"]), _resolve(rows, True, "unit_s2", st["block"], st["unit"])
            assert len(c2) == 1 and len(s2) == 1
            w2 = rows[c2[0]]
            assert (w2["N"], w2["taps"], w2["Cin"]) == (st["N"], 1, st["N"]) and rows[s2[0]]["d0"] == st["N"]
            used.update((c2[0], s2[0]))
    assert used == set(range(len(rows))), [rows[i]["base"] for i in set(range(len(rows))) - used]
    if name == "default":
        assert any(st["fused"] for st in plan["steps"])
