"""CPU: the checker of tests/test_vae_layers_gpu.py tested against an EMULATED kernel, without a GPU.

The emulation is what conv.hip computes, in torch fp32 on the same bf16 operands: Snake in fp32 with torch's fp32 sin (standing in for
v_sin_f32), fp32-accumulating convs, roundings at the native places.  The clean emulation must stay inside the elementwise bound of
tests/_vae_layers.py at a stage of every kind, and every seeded defect - the kind of local error a global relative L2 cannot see - must
put at least one element over it.  This is the proof that the GPU tests would notice a subtly wrong kernel.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import _vae_layers as vl

CFG_KW = dict(decoder_channels=128, channel_multiples=(1, 2), downsampling_ratios=(2, 4))
N_BLOCKS = 2


@pytest.fixture(scope="module")
def weights():
    import ace355
    from ace355 import weightgen
    cfg = ace355.VaeConfig(**CFG_KW)
    return weightgen.make_vae_weights({**cfg.weight_shapes(), **cfg.encoder_weight_shapes()}, seed=3, mode="test")


def _info(kind, block=-1, unit=-1, flags=0, dil=1):
    return dict(kind=kind, block=block, unit=unit, channels=0, flags=flags, src=-1, res=-1, dilation=dil, rows=0)


# name -> (encoder?, stage info, input channels, rows, stride).  One stage of each kind; the Snake-free ones first.
STAGES = {
    "dec.conv_in": (False, _info(vl.CONV_IN), 64, 333, 1),
    "dec.convt": (False, _info(vl.CONVT, block=0), 256, 150, 4),
    "enc.down": (True, _info(vl.DOWN, block=1), 128, 402, 4),
    "dec.unit_k1": (False, _info(vl.UNIT_K1, block=1, unit=0), 128, 333, 1),
    "dec.conv_in+osnake": (False, _info(vl.CONV_IN, flags=vl.OUT_SNAKE), 64, 333, 1),
    "dec.convt+isnake": (False, _info(vl.CONVT, block=0, flags=vl.IN_SNAKE), 256, 150, 4),
    "enc.down+isnake+osnake": (True, _info(vl.DOWN, block=1, flags=vl.IN_SNAKE | vl.OUT_SNAKE), 128, 402, 4),
    "dec.unit_fused": (False, _info(vl.UNIT, block=1, unit=1, flags=vl.FUSED | vl.IN_SNAKE, dil=3), 128, 333, 1),
    "dec.unit_fused+osnake": (False, _info(vl.UNIT, block=0, unit=2, flags=vl.FUSED | vl.IN_SNAKE | vl.OUT_SNAKE, dil=9), 128, 333, 1),
    "enc.unit_k7+osnake": (True, _info(vl.UNIT_K7, block=0, unit=2, flags=vl.IN_SNAKE | vl.OUT_SNAKE, dil=9), 128, 333, 1),
    "enc.unit_k7": (True, _info(vl.UNIT_K7, block=0, unit=1, flags=vl.IN_SNAKE, dil=3), 128, 333, 1),
    "dec.unit_k1+isnake+osnake": (False, _info(vl.UNIT_K1, block=1, unit=2, flags=vl.IN_SNAKE | vl.OUT_SNAKE), 128, 333, 1),
    "enc.head": (True, _info(vl.HEAD, flags=vl.F32_NCL | vl.IN_SNAKE), 256, 200, 1),
    "dec.out": (False, _info(vl.OUT, flags=vl.F32_NCL | vl.IN_SNAKE), 128, 333, 1),
    "dec.out_plain": (False, _info(vl.OUT, flags=vl.F32_NCL), 128, 333, 1),
}


def _snake32(x, w, p):
    a = torch.exp(w[p + ".alpha"].float().reshape(1, -1, 1))
    ib = 1.0 / (torch.exp(w[p + ".beta"].float().reshape(1, -1, 1)) + 1e-9)
    return x + ib * torch.sin(a * x).pow(2)


def _bf(x):
    return x.to(torch.bfloat16).float()


def emulate(w, enc, info, x64, res64, stride, defect=None):
    """The native layer in fp32 (see the module docstring), NCL [B, C, L]; ``defect`` seeds one local error."""
    k, flags = info["kind"], info["flags"]
    nm = vl._snake_names(enc, info, N_BLOCKS)
    x = x64.float()
    res = None if res64 is None else res64.float()
    W = vl.fused_weight(w, nm["conv"]).float()
    bias = w.get(nm["conv"] + ".bias")
    bias = None if bias is None else bias.float().clone()
    if defect == "flip_input":
        x = x.clone()
        x[0, 5, x.shape[2] // 2] *= -1
    if defect == "shift_input":
        x = F.pad(x, (1, 0))[:, :, :-1]
    # (a one-launch unit shows its k = 7 stage only through the k = 1 conv, which spreads one wrong k = 7 operand over 128 channels at
    #  1 / 128 of its size - under any bound on the output; its weight / bias defects are seeded in the k = 1 stage, and the k = 7 conv at
    #  the same width is held on its own where the unit runs as two launches: unit_k7, and the ACE355_CONV_FUSE_RU=0 runs on the GPU)
    if defect == "flip_weight" and k != vl.UNIT:
        W = W.clone()
        W[1, 7, W.shape[2] // 2] *= -1
    if defect == "no_bias_channel" and k != vl.UNIT:
        bias[11] = 0.0
    if defect == "res_row_above":
        res = F.pad(res, (1, 0))[:, :, :-1]
    if flags & vl.IN_SNAKE:
        x = _bf(_snake32(x, w, nm["in_snake"]))
    if k == vl.CONVT:
        y = F.conv_transpose1d(x, W, bias, stride=stride, padding=math.ceil(stride / 2))
    elif k == vl.DOWN:
        y = F.conv1d(x, W, bias, stride=stride, padding=math.ceil(stride / 2))
    else:
        d = info["dilation"]
        y = F.conv1d(x, W, bias, dilation=d, padding=(W.shape[2] // 2) * d)
    if k == vl.UNIT:
        u = _bf(_snake32(y, w, nm["mid_snake"]))
        W2, b2 = vl.fused_weight(w, nm["conv2"]).float().clone(), w[nm["conv2"] + ".bias"].float().clone()
        if defect == "flip_weight":
            W2[1, 7, 0] *= -1
        if defect == "no_bias_channel":
            b2[11] = 0.0
        y = F.conv1d(u, W2, b2) + res
    elif k == vl.UNIT_K1:
        y = y + res
    if flags & vl.OUT_SNAKE:
        y = _snake32(y, w, nm["out_snake"])
    if not (flags & vl.F32_NCL):
        y = _bf(y)
    y = y.clone()
    if defect == "drop_last_row":
        y[:, :, -1] = 0.0
    if defect == "zero_group":
        y[1, 16:24, y.shape[2] // 3] = 0.0
    return y.double()


def _inputs(name):
    enc, info, cin, rows, stride = STAGES[name]
    g = torch.Generator().manual_seed(len(name) + cin + rows)
    x = vl.bf16r(torch.randn(2, cin, rows, generator=g).double())
    res = vl.bf16r(torch.randn(2, cin, rows, generator=g).double()) if info["kind"] in (vl.UNIT, vl.UNIT_K1) else None
    return enc, info, x, res, stride


def _run(weights, name, defect=None):
    enc, info, x, res, stride = _inputs(name)
    ref, absref, K = vl.layer_reference(weights, enc, info, N_BLOCKS, x, res, stride)
    got = emulate(weights, enc, info, x, res, stride, defect)
    u = vl.U_F32 if info["flags"] & vl.F32_NCL else vl.U_BF16
    tau = vl.tau_for(info["kind"], info["flags"], K)
    return vl.compare(got, ref, absref, u, tau, f"{name}{' / ' + defect if defect else ''}"), tau, K


def test_constants_match_the_header():
    from ace355 import native
    assert (vl.INPUT, vl.CONV_IN, vl.CONVT, vl.UNIT, vl.UNIT_K7, vl.UNIT_K1, vl.DOWN, vl.HEAD) == (
        native.VAE_STAGE_INPUT, native.VAE_STAGE_CONV_IN, native.VAE_STAGE_CONVT, native.VAE_STAGE_UNIT, native.VAE_STAGE_UNIT_K7,
        native.VAE_STAGE_UNIT_K1, native.VAE_STAGE_DOWN, native.VAE_STAGE_HEAD)
    assert (vl.IN_SNAKE, vl.OUT_SNAKE, vl.FUSED, vl.F32_NCL) == (
        native.VAE_FLAG_IN_SNAKE, native.VAE_FLAG_OUT_SNAKE, native.VAE_FLAG_FUSED, native.VAE_FLAG_F32_NCL)
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ace355.h")).read()
    for cname, val in [("STAGE_INPUT", vl.INPUT), ("STAGE_CONV_IN", vl.CONV_IN), ("STAGE_CONVT", vl.CONVT), ("STAGE_UNIT", vl.UNIT),
                       ("STAGE_UNIT_K7", vl.UNIT_K7), ("STAGE_UNIT_K1", vl.UNIT_K1), ("STAGE_DOWN", vl.DOWN), ("STAGE_HEAD", vl.HEAD),
                       ("FLAG_IN_SNAKE", vl.IN_SNAKE), ("FLAG_OUT_SNAKE", vl.OUT_SNAKE), ("FLAG_FUSED", vl.FUSED), ("FLAG_F32_NCL", vl.F32_NCL)]:
        m = re.search(r"#define ACE355_VAE_%s (\d+)\b" % cname, hdr)
        assert m and int(m.group(1)) == val, cname


def test_tap_sum_is_the_conv():
    g = torch.Generator().manual_seed(0)
    for cin, cout, k, dil in [(16, 24, 7, 1), (16, 8, 7, 9), (32, 32, 1, 1), (8, 8, 3, 1)]:
        x = torch.randn(2, cin, 101, generator=g, dtype=torch.float64)
        w = torch.randn(cout, cin, k, generator=g, dtype=torch.float64)
        ref = F.conv1d(x, w, dilation=dil, padding=(k // 2) * dil)
        assert float((vl.conv_taps(x, w, dil) - ref).abs().max()) < 1e-12


def test_weight_fusion_follows_the_oracle(weights):
    """fused_weight restates the handle's fp32 fusion; against the oracle's fusion it may differ by fp32 rounding only."""
    from oracle import oobleck as o_vae
    for base in ("decoder.conv1", "decoder.block.0.conv_t1", "encoder.block.1.conv1"):
        a = vl.fused_weight(weights, base)
        b = o_vae._w(weights, base).double()
        assert a.shape == b.shape and float((a - b).abs().max()) <= 2.0 ** -8 * float(b.abs().max())


@pytest.mark.parametrize("name", list(STAGES))
def test_clean_emulation_passes(weights, name):
    r, tau, K = _run(weights, name)
    print(f"{name}: K {K}, tau {tau:.3g} (ceiling {vl.tau_ceiling(K):.3g}), measured excess {r['excess']:.3g} absref")
    assert r["n_over"] == 0, r["report"]
    if not vl.has_snake(STAGES[name][1]["flags"]):
        assert tau == 2.0 ** -21


GENERIC = ["flip_input", "flip_weight", "shift_input", "zero_group", "no_bias_channel"]
DEFECTS = ([(n, d) for n in ("dec.conv_in", "dec.convt", "enc.down", "dec.unit_k1", "dec.convt+isnake", "dec.unit_fused",
                             "dec.unit_fused+osnake", "enc.unit_k7+osnake", "enc.head") for d in GENERIC] +
           [("dec.out", d) for d in GENERIC if d not in ("no_bias_channel", "zero_group")] +    # (the output conv: no bias, 2 channels)
           [("dec.convt", "drop_last_row"), ("dec.convt+isnake", "drop_last_row")] +
           [(n, "res_row_above") for n in ("dec.unit_k1", "dec.unit_fused", "dec.unit_fused+osnake", "dec.unit_k1+isnake+osnake")])


@pytest.mark.parametrize("name,defect", DEFECTS)
def test_seeded_defect_fails(weights, name, defect):
    r, tau, K = _run(weights, name, defect)
    print(f"{name} / {defect}: {r['n_over']} elements over the bound (tau {tau:.3g})")
    assert r["n_over"] >= 1, f"{name}: the defect '{defect}' went unnoticed"
    assert "row" in r["report"] and "channel" in r["report"]


def test_a_global_l2_would_not_have_seen_it(weights):
    """Why the bound is elementwise: one sign-flipped input element of a k = 7 conv leaves the relative L2 where it was."""
    def rel(a, b):
        return float((a - b).norm() / b.norm())
    enc, info, x, res, stride = _inputs("enc.unit_k7")
    ref, _a, _K = vl.layer_reference(weights, enc, info, N_BLOCKS, x, res, stride)
    clean, bad = emulate(weights, enc, info, x, res, stride), emulate(weights, enc, info, x, res, stride, "flip_input")
    assert rel(bad, ref) < 6e-3 and rel(clean, ref) < 6e-3        # the tolerance test_conv1d_nlc held such a conv to
