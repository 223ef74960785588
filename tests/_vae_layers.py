"""Teacher-forced layer parity of the Oobleck VAE: the per-layer fp64 references and the elementwise bound (helper module, no tests here).

Every stage of a native decode / encode (``NativeVae.stages``) is the output of ONE ``conv_kernel`` launch.  ``stage_reference`` applies
that one layer in fp64 torch to the NATIVE tensor of the stage it reads (exact bf16 values, so a layer never inherits drift), rounds
where the native layer rounds (the stage flags say where: nothing is hard-coded here), and ``compare`` holds every element to

    |got - ref| <= u * |ref| + tau * absref

``ref`` carries every rounding INSIDE the layer (Snake values that become bf16 MFMA operands) but not the final rounding of the stored
tensor: that one rounding is the ``u |ref|`` term, ``u`` = 2^-8 for a bf16-stored stage (bf16's unit roundoff: round-to-nearest moves a
value by at most half the spacing, 2^-8 of its magnitude at the bottom of a binade), 2^-23 for an fp32 output.  ``absref``: the same layer on absolute values (|input| after its Snake, |weights|, |bias|, |residual|; for a one-launch
residual unit through both convs) - the magnitude the fp32 accumulation error scales with.  ``tau``: TAU_LINEAR for a layer without a
Snake inside the kernel, the measured table TAU_MEASURED for one with (see there).

The references are plain torch: ``F.conv_transpose1d`` / strided ``F.conv1d`` for the transposed / strided convs (the polyphase and
shifted-view forms of conv.hip are NOT restated), the defining tap sum for the stride-1 convs.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

Tensor = torch.Tensor

# ACE355_VAE_STAGE_* / ACE355_VAE_FLAG_* (include/ace355.h; tests/test_vae_layers_cpu.py checks them against ace355.native)
INPUT, CONV_IN, CONVT, UNIT, UNIT_K7, UNIT_K1, DOWN, HEAD = range(8)
OUT = 8   # the decoder's output conv (decoder.conv2): not a stored stage, its result is the call's waveform
KIND_NAMES = ["input", "conv_in", "convt", "unit(fused)", "unit_k7", "unit_k1", "down", "head", "out"]
IN_SNAKE, OUT_SNAKE, FUSED, F32_NCL = 1, 2, 4, 8

U_BF16 = 2.0 ** -8    # bf16 keeps 8 significant bits: spacing 2^-7 of the binade's low end, round-to-nearest error at most half of it
U_F32 = 2.0 ** -23
# Layers WITHOUT a Snake inside the kernel.  Derived, not measured: 8 x the fp32 unit roundoff (2^-24) on the accumulated magnitude -
# an fp32 sum of K products in the MFMA's blocked order stays far below K * 2^-24 * absref in practice (the fp32-accumulate emulation of
# tests/test_vae_layers_cpu.py shows <= 5.2e-8 * absref = 0.9 * 2^-24 at K = 896 ... 14336), plus the fp32 bias / residual adds.
TAU_LINEAR = 2.0 ** -21
# Layers WITH a Snake inside the kernel (input Snake rounded to bf16 in staging, snake2 between the two convs of a one-launch unit,
# producer-side Snake on the fp32 sum).  v_sin_f32 and the fp32 Snake arithmetic flip the bf16 rounding of some Snake values against the
# exact sin of the reference - each flip moves one of the K operands of an output by one bf16 step - and the producer-side Snake
# amplifies the sum's fp32 error by its slope.  Nothing is assumed about how often: the numbers below are the largest
# (|got - ref| - u |ref|) / absref MEASURED on an MI355X against the fp64 reference, per stage kind, Snake placement and K = taps * Cin
# (i.e. channel width), over every configuration of tests/test_vae_layers_gpu.py (child-process switches included) and the Snake cases of
# tests/test_kernels_gpu.py::test_conv1d_nlc (taps 7 -> UNIT_K7, taps 1 -> UNIT_K1).  tau = 4 x the measured maximum (the margin is for
# seeds, lengths and boards not measured), never below TAU_LINEAR, and never above the hard ceiling 1 / (4 K): a single typical wrong
# input element moves an output by ~ 2 absref / K, and above the ceiling the test could no longer see it.  Where 4 x the measurement
# exceeds the ceiling the ceiling is in force (tau_at_ceiling; listed in tests/perf/README.md, "VAE layer parity"): the k = 7 convs of
# the wide units sit at ~ 0.17 / K - about 35 flipped operands of 7168 per output, worst of 10^8 outputs - which leaves a factor 1.4.
# (kind, Snake on the MFMA operands?) -> {K: measured maximum}.  True: a Snake value is rounded to bf16 and fed to the MFMAs inside the launch
# (input Snake in staging, snake2 of a one-launch unit); False: only the producer-side Snake on the fp32 sum - those stay at fp32
# level (<= 1.2e-7) and are held to TAU_LINEAR like the Snake-free layers.
TAU_MEASURED: Dict[Tuple[int, bool], Dict[int, float]] = {
    (CONV_IN, False): {448: 1.396e-08},
    (CONVT, True): {256: 3.552e-04, 512: 7.654e-06},
    (UNIT, True): {896: 1.169e-04},
    (UNIT_K7, True): {448: 1.727e-04, 896: 7.365e-05, 1792: 9.719e-05, 3584: 4.755e-05, 7168: 2.450e-05},
    (UNIT_K1, True): {64: 7.668e-04, 128: 1.840e-04, 256: 4.820e-04},
    (UNIT_K1, False): {64: 1.189e-07, 128: 7.092e-08, 256: 9.788e-08, 512: 9.032e-08, 1024: 5.625e-08},
    (DOWN, True): {512: 1.665e-06, 1024: 1.918e-05, 3072: 1.153e-05},
    (DOWN, False): {3072: 3.432e-09, 20480: 6.073e-08},
    (HEAD, True): {1536: 8.321e-06},
    (OUT, True): {448: 5.807e-06},
}


def has_snake(flags: int) -> bool:
    return bool(flags & (IN_SNAKE | OUT_SNAKE | FUSED))


def tau_ceiling(K: int) -> float:
    return 1.0 / (4.0 * K)


def _tau_wanted(kind: int, flags: int, K: int) -> float:
    m = TAU_MEASURED.get((kind, bool(flags & (IN_SNAKE | FUSED))), {})
    meas = m.get(K, max(m.values()) if m else 0.0)   # a width that was not measured: the largest measurement of its class
    return max(4.0 * meas, TAU_LINEAR)


def tau_at_ceiling(kind: int, flags: int, K: int) -> bool:
    return has_snake(flags) and _tau_wanted(kind, flags, K) > tau_ceiling(K)


def tau_for(kind: int, flags: int, K: int) -> float:
    """The tau in force for a stage.  The ceiling is never exceeded: a stage that needs more fails, it is not given more."""
    if not has_snake(flags):
        return TAU_LINEAR
    return min(_tau_wanted(kind, flags, K), tau_ceiling(K))


# ------------------------------------------------------------------------------------------------ arithmetic
def bf16r(x: Tensor) -> Tensor:
    """Round to bf16 (nearest even), back in fp64."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def snake64(x: Tensor, alpha: Tensor, beta: Tensor) -> Tensor:
    """x + 1 / (exp(beta) + 1e-9) * sin(exp(alpha) x)^2 in fp64 with the exact sin; x [B, C, L], parameters any shape with C elements."""
    a = torch.exp(alpha.double().reshape(1, -1, 1))
    ib = 1.0 / (torch.exp(beta.double().reshape(1, -1, 1)) + 1e-9)
    return x + ib * torch.sin(a * x).pow(2)


def fused_weight(w: Dict[str, Tensor], base: str) -> Tensor:
    """The weight the handle holds: weight-norm fused in fp32 (g * v / (||v|| + 1e-9), the norm accumulated in fp64 and rounded to
    fp32, over all dims but 0 - Conv1d and ConvTranspose1d alike) and rounded to bf16.  fp64 values, the state dict's layout."""
    if base + ".weight" in w:
        return bf16r(w[base + ".weight"].double())
    v = w[base + ".weight_v"].float()
    g = w[base + ".weight_g"].float().reshape(-1, 1, 1)
    nrm = v.double().reshape(v.shape[0], -1).pow(2).sum(1).sqrt().float().reshape(-1, 1, 1)
    return ((g * v) / (nrm + torch.tensor(1e-9, dtype=torch.float32))).to(torch.bfloat16).to(torch.float64)


def conv_taps(x: Tensor, w: Tensor, dil: int = 1) -> Tensor:
    """Stride-1 'same' Conv1d by its definition, y[b, :, l] = sum_k w[:, :, k] @ x[b, :, l + (k - K//2) dil] (zero outside): one fp64
    GEMM per tap.  Equal to F.conv1d(x, w, dilation=dil, padding=(K // 2) * dil) (checked on the CPU), several times faster for wide,
    short layers."""
    K = w.shape[2]
    L = x.shape[2]
    pad = (K // 2) * dil
    xp = F.pad(x, (pad, pad))
    y = torch.zeros(x.shape[0], w.shape[0], L, dtype=x.dtype)
    for k in range(K):
        y += torch.matmul(w[:, :, k], xp[:, :, k * dil:k * dil + L])
    return y


def _lin(kind: str, x: Tensor, w: Tensor, bias: Optional[Tensor], stride: int, dil: int) -> Tensor:
    if kind == "convt":
        y = F.conv_transpose1d(x, w, None, stride=stride, padding=math.ceil(stride / 2))
    elif kind == "strided":
        y = F.conv1d(x, w, None, stride=stride, padding=math.ceil(stride / 2))
    else:
        y = conv_taps(x, w, dil)
    if bias is not None:
        y = y + bias.reshape(1, -1, 1)
    return y


def linear_pair(kind: str, x: Tensor, w: Tensor, bias: Optional[Tensor], stride: int = 1, dil: int = 1,
                res: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(conv(x, w) + bias + res, the same on absolute values), fp64."""
    b64 = None if bias is None else bias.double()
    y = _lin(kind, x, w, b64, stride, dil)
    a = _lin(kind, x.abs(), w.abs(), None if b64 is None else b64.abs(), stride, dil)
    if res is not None:
        y = y + res
        a = a + res.abs()
    return y, a


# ------------------------------------------------------------------------------------------------ per-stage references
def _snake_names(enc: bool, info: Dict[str, int], n_blocks: int) -> Dict[str, Optional[str]]:
    """Parameter-name prefixes of a stage's layer: conv(s), the Snake ahead of the conv, and the reader's Snake a producer applies."""
    side = "encoder" if enc else "decoder"
    k, b, j = info["kind"], info["block"], info["unit"]
    blk = f"{side}.block.{b}"
    ru = f"{blk}.res_unit{j + 1}"
    # the single reader of a block's last unit: decoder -> the next block's transposed conv (or the output conv); encoder -> the block's
    # own strided conv
    after_unit3 = (f"{blk}.snake1" if enc else (f"{side}.block.{b + 1}.snake1" if b + 1 < n_blocks else f"{side}.snake1"))
    if k == CONV_IN:
        return dict(conv=f"{side}.conv1", in_snake=None, out_snake=None if enc else f"{side}.block.0.snake1")
    if k == CONVT:
        return dict(conv=f"{blk}.conv_t1", in_snake=f"{blk}.snake1", out_snake=None)
    if k == DOWN:
        return dict(conv=f"{blk}.conv1", in_snake=f"{blk}.snake1", out_snake=f"{side}.snake1")
    if k == UNIT:
        return dict(conv=f"{ru}.conv1", conv2=f"{ru}.conv2", in_snake=f"{ru}.snake1", mid_snake=f"{ru}.snake2", out_snake=after_unit3)
    if k == UNIT_K7:
        return dict(conv=f"{ru}.conv1", in_snake=f"{ru}.snake1", out_snake=f"{ru}.snake2")
    if k == UNIT_K1:
        return dict(conv=f"{ru}.conv2", in_snake=f"{ru}.snake2", out_snake=after_unit3)
    if k in (HEAD, OUT):
        return dict(conv=f"{side}.conv2", in_snake=f"{side}.snake1", out_snake=None)
    raise ValueError(k)


def layer_reference(w: Dict[str, Tensor], enc: bool, info: Dict[str, int], n_blocks: int, x: Tensor, res: Optional[Tensor],
                    stride: int = 1) -> Tuple[Tensor, Tensor, int]:
    """One layer in fp64.  x / res: the native tensors the launch reads, NCL fp64 [B, C, L] (exact bf16 values; for the encoder's first
    conv the bf16-rounded audio).  Returns (ref, absref, K): ref is the value ahead of the stage's final rounding, absref is the
    magnitude sum of the layer's last conv, K = taps * Cin of the stage's (first) conv as the kernel sees it."""
    k, flags = info["kind"], info["flags"]
    nm = _snake_names(enc, info, n_blocks)
    sn = lambda t, p: snake64(t, w[p + ".alpha"], w[p + ".beta"])
    W = fused_weight(w, nm["conv"])
    bias = w.get(nm["conv"] + ".bias")
    if flags & IN_SNAKE:
        x = bf16r(sn(x, nm["in_snake"]))   # the window staging rounds snake(x) to bf16 ahead of the MFMAs
    if k == CONVT:
        y, a = linear_pair("convt", x, W, bias, stride=stride)
        K = 2 * W.shape[0]                    # two input rows per output sample
    elif k == DOWN:
        y, a = linear_pair("strided", x, W, bias, stride=stride)
        K = W.shape[1] * W.shape[2]
    elif k == UNIT:
        t, ta = linear_pair("conv", x, W, bias, dil=info["dilation"])      # k = 7 result, kept unrounded ...
        u = bf16r(sn(t, nm["mid_snake"]))                                   # ... up to snake2, whose value is the k = 1 stage's bf16 operand
        ua = torch.maximum(u.abs(), sn(ta, nm["mid_snake"]))                # magnitude through snake2: the Snake of the magnitude sum
        W2 = fused_weight(w, nm["conv2"])
        b2 = w[nm["conv2"] + ".bias"].double()
        y = _lin("conv", u, W2, b2, 1, 1) + res
        a = _lin("conv", ua, W2.abs(), b2.abs(), 1, 1) + res.abs()
        K = W.shape[1] * W.shape[2]
    else:
        y, a = linear_pair("conv", x, W, bias, dil=info["dilation"], res=res if k == UNIT_K1 else None)
        K = W.shape[1] * W.shape[2]
    if flags & OUT_SNAKE:
        y = sn(y, nm["out_snake"])            # the producer applies its reader's Snake to the fp32 sum; the store then rounds once
    # (the stage's own final rounding to bf16 is NOT applied: it is the u |ref| term of the bound)
    return y, a, K


# ------------------------------------------------------------------------------------------------ the comparison
def compare(got: Tensor, ref: Tensor, absref: Tensor, u: float, tau: float, label: str = "", max_lines: int = 8) -> Dict[str, object]:
    """Every element of got / ref / absref (NCL fp64 [B, C, L]) against the bound.  Returns the count of elements over it, the measured
    excess max((|got - ref| - u |ref|) / absref) (the quantity a Snake tau is set from) and a report of the worst offenders: item, row,
    channel, the row's position in its 128- and 256-row tile, got / ref / bound."""
    assert got.shape == ref.shape == absref.shape, (got.shape, ref.shape, absref.shape)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))   # a NaN / Inf anywhere is over every bound
    floor = absref.clamp_min(1e-300)
    excess = float(((err - u * ref.abs()) / floor).max())
    bound = u * ref.abs() + tau * absref
    over = err > bound
    n_over = int(over.sum())
    lines: List[str] = []
    if n_over:
        ratio = torch.where(over, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        worst = torch.topk(ratio.flatten(), min(max_lines, n_over)).indices
        C, L = got.shape[1], got.shape[2]
        for i in worst.tolist():
            b, c, l = i // (C * L), (i // L) % C, i % L
            lines.append(f"  {label}: item {b} row {l} (row {l % 128} of its 128-row tile, {l % 256} of its 256-row tile) channel {c} "
                         f"(8-channel group {c // 8}): got {float(got[b, c, l]):.9g} ref {float(ref[b, c, l]):.9g} "
                         f"bound {float(bound[b, c, l]):.3g} (x{float(ratio[b, c, l]):.2f})")
        lines.insert(0, f"{label}: {n_over} of {got.numel()} elements over |got - ref| <= {u:.3g} |ref| + {tau:.3g} absref")
    return {"n_over": n_over, "excess": excess, "report": "\n".join(lines)}


def to_ncl64(t: Tensor, f32_ncl: bool = False) -> Tensor:
    """A stored stage (bf16 [B, rows, channels], or f32 [B, channels, rows]) as fp64 [B, C, L] on the CPU."""
    t = t.detach().cpu()
    return t.double() if f32_ncl else t.double().transpose(1, 2).contiguous()


# ------------------------------------------------------------------------------------------------ one configuration on the GPU
def _stride_of(cfg, enc: bool, block: int) -> int:
    return int(cfg.downsampling_ratios[block] if enc else cfg.upsampling_ratios[block])


def run_case(cfg_kw: dict, enc: bool, B: int, frames: int, items: List[int], seed: int = 1, device: str = "cuda:0") -> Dict[str, object]:
    """Every stage of one native decode (z [B, 64, frames]) or encode (audio [B, 2, hop * frames]) against its fp64 layer reference on
    ``items``.  Returns {"records": one dict per compared stage (kind, channels, flags, K, tau, ceiling, excess, n_over), "reports":
    the failure reports, "errors": other broken assertions (tapped != untapped bits, an inexact input image)}; asserts nothing itself,
    so that one run lists every stage.  The A/B switches of the process (ACE355_VAE_EPISNAKE, ACE355_CONV_FUSE_RU, ...) apply."""
    import ace355
    from ace355 import weightgen
    from ace355.vae import NativeVae
    cfg = ace355.VaeConfig(**cfg_kw)
    w = weightgen.make_vae_weights({**cfg.weight_shapes(), **cfg.encoder_weight_shapes()}, seed=seed, mode="test")
    vae = NativeVae(cfg, device)
    vae.load_state_dict(w)
    nb = len(cfg.downsampling_ratios)
    g = torch.Generator().manual_seed(1000 * seed + frames)
    if enc:
        T = cfg.hop * frames
        call_in = 0.3 * torch.randn(B, cfg.audio_channels, T, generator=g)
        call = lambda: vae.encode(call_in, sample=False)
    else:
        T = frames
        call_in = torch.randn(B, cfg.decoder_input_channels, T, generator=g)
        call = lambda: vae.decode(call_in)
    errors: List[str] = []
    stages = vae.stages(enc, T)
    plain = call().cpu()
    bufs = [vae.stage_buffer(si, B) for si in stages]
    for k, buf in enumerate(bufs):
        buf.zero_()
        vae.set_tap(enc, k, buf)
    tapped = call().cpu()
    torch.cuda.synchronize()
    for k in range(len(stages)):
        vae.set_tap(enc, k, None)
    if not torch.equal(plain, tapped):
        errors.append("the tapped call's output differs from the untapped call's")
    if not torch.equal(call().cpu(), plain):
        errors.append("the call after the taps were cleared differs from the first")
    idx = torch.tensor(items)
    in64 = bf16r(call_in[idx].double())                 # both halves round the call's fp32 input to bf16 first
    cache: Dict[int, Tensor] = {}

    def stage_tensor(k: int) -> Tensor:
        if k not in cache:
            cache[k] = to_ncl64(bufs[k][idx.to(bufs[k].device)], bool(stages[k]["flags"] & F32_NCL))
        return cache[k]

    records, reports = [], []

    def one(info, x, res, got, label, stride):
        ref, absref, K = layer_reference(w, enc, info, nb, x, res, stride)
        f32 = bool(info["flags"] & F32_NCL)
        tau = tau_for(info["kind"], info["flags"], K)
        r = compare(got, ref, absref, U_F32 if f32 else U_BF16, tau, label)
        records.append(dict(label=label, kind=info["kind"], channels=int(got.shape[1]), rows=int(got.shape[2]), flags=info["flags"], K=K, tau=tau,
                            ceiling=tau_ceiling(K), excess=r["excess"], n_over=r["n_over"], elements=got.numel()))
        if r["n_over"]:
            reports.append(r["report"])

    for k, si in enumerate(stages):
        label = f"{'enc' if enc else 'dec'} stage {k} {KIND_NAMES[si['kind']]} block {si['block']} unit {si['unit']} C={si['channels']} flags={si['flags']}"
        got = stage_tensor(k)
        if si["kind"] == INPUT:
            if enc:    # im2col rows: column k * A + c = audio[c][l + k - 3], zero outside and in the padding columns
                A = cfg.audio_channels
                xp = F.pad(in64, (3, 3))
                want = torch.zeros_like(got)
                for tap in range(7):
                    want[:, tap * A:(tap + 1) * A] = xp[:, :, tap:tap + T]
            else:
                want = in64
            if not torch.equal(got, want):
                errors.append(f"{label}: the input image is not the bf16-rounded input ({int((got != want).sum())} elements differ)")
            records.append(dict(label=label, kind=INPUT, channels=int(got.shape[1]), rows=int(got.shape[2]), flags=0, K=0, tau=0.0, ceiling=0.0,
                                excess=0.0, n_over=int((got != want).sum()), elements=got.numel()))
            continue
        x = in64 if (enc and si["kind"] == CONV_IN) else stage_tensor(si["src"])
        res = stage_tensor(si["res"]) if si["res"] >= 0 else None
        stride = _stride_of(cfg, enc, si["block"]) if si["kind"] in (CONVT, DOWN) else 1
        one(si, x, res, got, label, stride)
        for old in [j for j in cache if j < k - 3]:
            del cache[old]
    last = stages[-1]
    if enc:
        Z = cfg.decoder_input_channels
        if not torch.equal(plain[idx].double(), stage_tensor(len(stages) - 1)[:, :Z]):
            errors.append("encode(sample=False) is not the mean half of the head")
        # the sampled latent: mean + (softplus(scale) + 1e-4) * noise from the native head, fp32 arithmetic on three terms
        noise = torch.randn(B, Z, frames, generator=g)
        z = vae.encode(call_in, noise=noise).cpu()[idx].double()
        head = stage_tensor(len(stages) - 1)
        std = F.softplus(head[:, Z:]) + 1e-4
        zref = head[:, :Z] + std * noise[idx].double()
        r = compare(z, zref, head[:, :Z].abs() + std * noise[idx].double().abs(), U_F32, 2.0 ** -21, "enc latents = mean + std * noise")
        records.append(dict(label="enc gaussian head", kind=HEAD, channels=Z, rows=frames, flags=F32_NCL, K=0, tau=2.0 ** -21, ceiling=0.0,
                            excess=r["excess"], n_over=r["n_over"], elements=z.numel()))
        if r["n_over"]:
            reports.append(r["report"])
    else:
        info = dict(kind=OUT, block=-1, unit=-1, channels=cfg.audio_channels, dilation=1, src=len(stages) - 1, res=-1,
                    flags=F32_NCL | (0 if last["flags"] & OUT_SNAKE else IN_SNAKE))
        one(info, stage_tensor(len(stages) - 1), None, plain[idx].double(), f"dec output conv C={cfg.audio_channels} flags={info['flags']}", 1)
    vae.close()
    return {"records": records, "reports": reports, "errors": errors, "n_stages": len(stages),
            "kinds": [s["kind"] for s in stages], "stage_flags": [s["flags"] for s in stages]}


def summarize(tag: str, out: Dict[str, object]) -> str:
    """Per stage kind, channel width and Snake placement: the measured excess over u |ref| in units of absref, and the tau in force."""
    rows: Dict[Tuple[int, int, bool], List[dict]] = {}
    for r in out["records"]:
        if r["kind"] != INPUT:
            rows.setdefault((r["kind"], r["channels"], has_snake(r["flags"]) if r["K"] else False), []).append(r)
    lines = [f"[{tag}] {out['n_stages']} stages, {len(out['records'])} comparisons"]
    for (kind, ch, sn), rs in sorted(rows.items()):
        lines.append(f"[{tag}]   {KIND_NAMES[kind]:12s} C={ch:<5d} {'snake ' if sn else 'linear'} x{len(rs)}: max excess {max(r['excess'] for r in rs):10.3e} absref, "
                     f"tau {rs[0]['tau']:.3e}{' (AT THE CEILING)' if sn and rs[0]['tau'] >= rs[0]['ceiling'] else ''}, "
                     f"ceiling 1/(4K) {rs[0]['ceiling']:.3e}, over the bound {sum(r['n_over'] for r in rs)}")
    return "\n".join(lines)


if __name__ == "__main__":   # child process of tests/test_vae_layers_gpu.py: the A/B switches are read once per process
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    spec = json.loads(sys.argv[1])
    kw = {k: tuple(v) if isinstance(v, list) else v for k, v in spec["cfg_kw"].items()}
    res = run_case(kw, spec["enc"], spec["B"], spec["frames"], spec["items"])
    with open(sys.argv[2], "w") as f:
        json.dump(res, f)
