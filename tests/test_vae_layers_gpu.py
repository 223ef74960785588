"""GPU: teacher-forced layer parity of the native Oobleck VAE - every stored stage of a decode / encode against an fp64 reference of
that ONE layer applied to the native tensor it read, element by element (tests/_vae_layers.py; its checker is proven on the CPU by
tests/test_vae_layers_cpu.py).  Each comparison is one ``conv_kernel`` launch at the shapes and with the argument arithmetic the
product really uses, so the launch forms of ``launch_conv`` that whole decodes only reach at 30 dB are each held to

    |got - ref| <= u |ref| + tau absref        (u = 2^-8 bf16 / 2^-23 fp32; tau: _vae_layers.tau_for)

Launch forms per case, re-derived from launch_conv (wgs128 = ceil(M / 128) * ceil(N / 128) * B; 8-wave 256-row tile: k >= 3 convs with
Cin >= 128 and no residual from wgs128 >= 1400, the one-launch unit from 1400, plain-row transposed convs from 1500; N < 128: the
32-column tile; rasterisation when there is more than one column tile):

  small  B=2 T=37   widths 256 / 128 / 64, ratios 6 / 4 / 2, odd lengths (37, 222, 888, 1776): ragged last tiles everywhere; C = 64 units
                    and the output conv (N = 2) on the 32-column tile; C = 128 units as one launch on the 4-wave tile; transposed convs
                    cropped by y_shift / y_valid with M = L + 1; everything else 4-wave (largest wgs128 = 14 * 1 * 2).  Re-run in child
                    processes with ACE355_VAE_EPISNAKE=0 (every Snake in its reader's staging, an extra rounding of the k = 7 result)
                    and ACE355_CONV_FUSE_RU=0 (C = 128 units as two launches), so those launches get the same treatment.
  full   B=1 T=24   widths 2048 ... 128: every 4-wave form (largest wgs128: block 0's transposed conv, 1 * 80 * 1 = 80; k = 7 at C = 1024:
                    2 * 8 = 16; one-launch units at C = 128: 180 and 360 < 1400 -> 4-wave, snake2 through the LDS image).  Rasterisation
                    with tiles_m < 8 - the tail-only path - at block 0 (tiles_m = 1 x 80 column tiles, units 2 x 8) and block 1's
                    transposed conv (2 x 24); full groups of 8 row blocks plus a tail at block 1's units (12 x 4), block 2 (12 x 8,
                    units 45 x 2) and block 3's transposed conv (46 x 4).
  full   B=8 T=280  every decoder launch on the form of the 8 x 30 s metric run.  Block 0: transposed conv M = 281 -> 3 * 80 * 8 = 1920
                    >= 1500: tall; k = 7 at C = 1024, M = 2800 -> 22 * 8 * 8 = 1408 >= 1400: tall (the threshold is T >= 269: 21 row
                    tiles give 1344).  Block 1: 22 * 24 * 8 = 4224 and 132 * 4 * 8 = 4224; block 2: 132 * 8 * 8 and 525 * 2 * 8; block 3:
                    526 * 4 * 8, units 2100 * 8 = 16800 >= 1400: the 8-wave one-launch unit (snake2 from the accumulators); block 4:
                    2101 * 2 * 8, units 4200 * 8.  conv1 (Cin = 64) and the k = 1 convs (residual) stay 4-wave by design; the output conv
                    is the 32-column tile.  Reference on items 0 and 7 (items are independent: bit-tested in tests/test_vae_gpu.py).
  enc    B=2 12 frames   L = 23040: im2col'ed first conv, one-launch units at C = 128 (4-wave: 180 * 2 = 360), k = 7 / k = 1 pairs at
                    C = 256 / 512 / 1024, the strided convs over the shifted flat view (x_shift, x_valid; never tall), the fp32 head.
  enc    B=4 188 frames  L = 360960: k = 7 at C = 256 (M = 45120 -> 353 * 2 * 4 = 2824) and C = 512 (M = 11280 -> 89 * 4 * 4 = 1424) on
                    the 8-wave tile, the one-launch units at C = 128 on the 8-wave form (2820 * 4, 1410 * 4); C = 1024 (M = 1880 ->
                    15 * 8 * 4 = 480) stays 4-wave.  Reference on item 3.
"""
import json
import os
import subprocess
import sys
import tempfile

import pytest

import _vae_layers as vl

pytestmark = pytest.mark.gpu

SMALL = dict(decoder_channels=64, channel_multiples=(1, 2, 4), downsampling_ratios=(2, 4, 6))


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
def test_decoder_layers(gpu_device, cfg_kw, B, T, items):
    out = vl.run_case(cfg_kw, False, B, T, items, device=str(gpu_device))
    _judge(f"dec {cfg_kw and 'small' or 'full'} B={B} T={T}", out, [vl.CONV_IN, vl.CONVT, vl.UNIT, vl.UNIT_K7, vl.UNIT_K1])


@pytest.mark.parametrize("cfg_kw,B,frames,items", [
    (SMALL, 2, 23, [0, 1]),
    (dict(), 2, 12, [0, 1]),
    (dict(), 4, 188, [3]),
], ids=["small-B2-23", "full-B2-12", "full-B4-188"])
def test_encoder_layers(gpu_device, cfg_kw, B, frames, items):
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
