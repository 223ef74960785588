"""GPU: teacher-forced layer parity of the native Oobleck VAE - every stored stage of a decode / encode against an fp64 reference of
that ONE layer applied to the native tensor it read, element by element (tests/_vae_layers.py; its checker is proven on the CPU by
tests/test_vae_layers_cpu.py).  Each comparison is one ``conv_kernel`` launch at the shapes and with the argument arithmetic the
product really uses, so the launch forms of ``launch_conv`` that whole decodes only reach at 30 dB are each held to

    |got - ref| <= u |ref| + tau absref        (u = 2^-8 bf16 / 2^-23 fp32; tau: _vae_layers.tau_for)

Which launch form every layer of a case takes is not derived here: tests/_vae_plan_cases.py LAYER_CASES states it per case (with the
tile counts that put it there), tests/test_vae_plan_cpu.py holds the statement to the library's plan_conv on any machine, and each test
below asserts it against ``native.vae_plan`` - the step list the decode / encode is about to execute - before it launches.  In short:

  small  B=2 T=37   odd lengths (37, 222, 888, 1776): ragged last tiles everywhere; C = 64 units and the output conv (N = 2) on the
                    32-column tile; C = 128 units as one launch on the 4-wave tile; transposed convs cropped by y_shift / y_valid with
                    M = L + 1.  Re-run in child processes with ACE355_VAE_EPISNAKE=0 and ACE355_CONV_FUSE_RU=0.
  full   B=1 T=24   every 4-wave form of the full widths; rasterisation with fewer than 8 row blocks (the tail-only path) and with full
                    groups of 8 plus a tail.
  full   B=8 T=280  every decoder launch on the form of the 8 x 30 s metric run (8-wave tiles, the 8-wave one-launch unit).  Reference on
                    items 0 and 7 (items are independent: bit-tested in tests/test_vae_gpu.py).
  enc    B=2 12 frames   im2col'ed first conv, one-launch units, k = 7 / k = 1 pairs, the strided convs over the shifted flat view
                    (x_shift, x_valid; never tall), the fp32 head: all 4-wave.
  enc    B=4 188 frames  k = 7 at C = 256 / 512 and the one-launch units on the 8-wave forms; C = 1024 stays 4-wave.  Reference on item 3.
"""
import json
import os
import subprocess
import sys
import tempfile

import pytest

import _vae_layers as vl
import _vae_plan_cases as plan_cases

pytestmark = pytest.mark.gpu

SMALL = plan_cases.SMALL
CLAIMS = {cid: (kw, enc, B, fr, default, special) for cid, kw, enc, B, fr, default, special in plan_cases.LAYER_CASES}


def _assert_claimed_forms(cid, cfg_kw, enc, B, frames):
    """The launches this case is about to make are on the forms tests/_vae_plan_cases.py claims for it."""
    kw, c_enc, c_B, c_fr, default, special = CLAIMS[cid]
    assert (kw, c_enc, c_B, c_fr) == (cfg_kw, enc, B, frames), "the case table and this test's parameters differ"
    plan_cases.assert_forms(plan_cases.vae_call(cfg_kw, enc, B, frames), default, special, cid)


def _judge(tag, out, expect_kinds=None):
    print(vl.summarize(tag, out))
    for rep in out["reports"]:
        print(rep)
    for e in out["errors"]:
        print(f"[{tag}] ERROR {e}")
    # every stage is tapped and compared, none skipped: one record per stage (+ the output conv / the Gaussian head)
    assert len(out["records"]) == out["n_stages"] + 1, (len(out["records"]), out["n_stages"])
    if expect_kinds is not None:
        for k in expect_kinds:
            assert k in out["kinds"], f"{tag}: no stage of kind {vl.KIND_NAMES[k]} in this process"
    assert not out["errors"], out["errors"]
    bad = [r for r in out["records"] if r["n_over"]]
    assert not bad, f"{tag}: {len(bad)} stages over the bound: " + "; ".join(f"{r['label']} ({r['n_over']} of {r['elements']})" for r in bad)


@pytest.mark.parametrize("cfg_kw,B,T,items", [
    (SMALL, 2, 37, [0, 1]),
    (dict(), 1, 24, [0]),
    (dict(), 8, 280, [0, 7]),
], ids=["small-B2-T37", "full-B1-T24", "full-B8-T280"])
def test_decoder_layers(gpu_device, request, cfg_kw, B, T, items):
    _assert_claimed_forms(request.node.callspec.id, cfg_kw, False, B, T)
    out = vl.run_case(cfg_kw, False, B, T, items, device=str(gpu_device))
    _judge(f"dec {cfg_kw and 'small' or 'full'} B={B} T={T}", out, [vl.CONV_IN, vl.CONVT, vl.UNIT, vl.UNIT_K7, vl.UNIT_K1])


@pytest.mark.parametrize("cfg_kw,B,frames,items", [
    (SMALL, 2, 23, [0, 1]),
    (dict(), 2, 12, [0, 1]),
    (dict(), 4, 188, [3]),
], ids=["small-B2-23", "full-B2-12", "full-B4-188"])
def test_encoder_layers(gpu_device, request, cfg_kw, B, frames, items):
    _assert_claimed_forms(request.node.callspec.id, cfg_kw, True, B, frames)
    out = vl.run_case(cfg_kw, True, B, frames, items, device=str(gpu_device))
    _judge(f"enc {cfg_kw and 'small' or 'full'} B={B} frames={frames}", out, [vl.CONV_IN, vl.UNIT, vl.UNIT_K7, vl.UNIT_K1, vl.DOWN, vl.HEAD])


@pytest.mark.parametrize("enc,frames", [(False, 37), (True, 23)], ids=["dec", "enc"])
@pytest.mark.parametrize("env", [{"ACE355_VAE_EPISNAKE": "0"}, {"ACE355_CONV_FUSE_RU": "0"},
                                 {"ACE355_VAE_EPISNAKE": "0", "ACE355_CONV_FUSE_RU": "0"}],
                         ids=["episnake0", "fuse0", "episnake0-fuse0"])
def test_switched_launches_get_the_same_treatment(gpu_device, env, enc, frames):
    """The small configuration with the Snakes in their readers' staging and / or every unit as two launches (switches read once per
    process: a child process under its own time limit)."""
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_vae_layers.py")
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "out.json")
        spec = dict(cfg_kw=SMALL, enc=enc, B=2, frames=frames, items=[0, 1])
        subprocess.run([sys.executable, helper, json.dumps(spec), path], check=True, env=dict(os.environ, **env), timeout=600)
        with open(path) as f:
            out = json.load(f)
    if "ACE355_CONV_FUSE_RU" in env:
        assert vl.UNIT not in out["kinds"], "the switch did not split the units"
    if "ACE355_VAE_EPISNAKE" in env:
        assert not any(f & vl.OUT_SNAKE for f in out["stage_flags"]), "the switch did not move the Snakes to their readers"
    _judge(f"{'enc' if enc else 'dec'} small {' '.join(f'{k}={v}' for k, v in env.items())}", out)


def test_tap_refuses_a_split_plan(gpu_device):
    """A tap is honoured on a whole-sequence, single-window plan only: under a budget that splits the decode the call fails
    (ACE355_ERR_STATE) instead of tapping one window; with the tap cleared the same decode runs, split, to the same bits."""
    import torch
    import ace355
    from ace355 import weightgen
    from ace355.vae import NativeVae
    cfg = ace355.VaeConfig(**SMALL)
    w = weightgen.make_vae_weights({**cfg.weight_shapes(), **cfg.encoder_weight_shapes()}, seed=1, mode="test")
    vae = NativeVae(cfg, gpu_device)
    vae.load_state_dict(w)
    z = torch.randn(2, 64, 200, generator=torch.Generator().manual_seed(9))
    whole = vae.decode(z).cpu()
    audio = 0.3 * torch.randn(2, 2, cfg.hop * 20, generator=torch.Generator().manual_seed(10))
    mean = vae.encode(audio, sample=False).cpu()
    plan = vae.decode_plan(2, 200)
    vae.set_decode_budget(plan["activation_bytes"] // 4)
    assert vae.decode_plan(2, 200)["core_frames"] < 200 or vae.decode_plan(2, 200)["items_per_window"] < 2
    si = vae.stage_info(False, 1, 200)
    buf = vae.stage_buffer(si, 2)
    vae.set_tap(False, 1, buf)
    with pytest.raises(RuntimeError, match="window"):
        vae.decode(z)
    esi = vae.stage_info(True, 1, cfg.hop * 20)
    ebuf = vae.stage_buffer(esi, 2)
    vae.set_decode_budget(cfg.hop * 20 * 128 * 2 * 3 + cfg.hop * 20 * 64 * 2)   # one item per encode group
    vae.set_tap(True, 1, ebuf)
    with pytest.raises(RuntimeError, match="window"):
        vae.encode(audio, sample=False)
    vae.set_tap(False, 1, None)
    vae.set_tap(True, 1, None)
    assert torch.equal(vae.encode(audio, sample=False).cpu(), mean)
    vae.set_decode_budget(plan["activation_bytes"] // 4)
    assert torch.equal(vae.decode(z).cpu(), whole)
    with pytest.raises(RuntimeError, match="stage"):
        vae.set_tap(False, vae.num_stages(False), buf)
    small = torch.empty(16, device=gpu_device, dtype=torch.bfloat16)
    vae.set_decode_budget(96 << 30)
    vae.set_tap(False, 1, small)
    with pytest.raises(RuntimeError, match="smaller"):
        vae.decode(z)
    vae.set_tap(False, 1, None)
    assert torch.equal(vae.decode(z).cpu(), whole)
    vae.close()
