#!/usr/bin/env python
"""The bits the native DiT computes, as SHA-256 lines: run it on two builds and compare the outputs line for line.

Only the public Python API is used (NativeDit.forward / cross_attention_maps, generate_latents, the handle's setters), so the same file runs
on any build.  Weights and inputs are seeded and generated on the CPU.  Cases:

  * tiny (256 wide, two layers; T = 37, two songs, L = 5): plain forward; CFG sampler with 4 steps; the same with a cover switch onto
    conditions of another length; SDE; no CFG; cross-attention maps of both layers and of layer 0 alone
  * mid (1024 wide, two layers; one song with CFG at T = 200: 200 rows): the sampler with folded norms
  * wide (2048 wide, two layers; four sequences at T = 768: 1536 rows, the smallest that reaches the MX path): forward and no-CFG sampler in
    the MXFP8 precision
each under the default switches and under the settings of SETTINGS - one child process per setting, the switches are read once.  The run
stops at the first child that fails.
Usage: python tools/dit_bits.py [--out FILE] [--root DIR]     (DIR: the checkout to import, default this file's)
"""
from __future__ import annotations

import argparse
import hashlib
import os
import subprocess
import sys

SETTINGS = [{}, {"ACE355_NORM_FOLD": "0"}, {"ACE355_NORM_FOLD": "2"}, {"ACE355_DEDUP0": "0"}, {"ACE355_GEMM_ZROW": "0"}, {"ACE355_SCHED_TABLES": "0"},
            {"ACE355_GEMM_PF": "0"}, {"ACE355_DUAL": "0"}, {"ACE355_DUAL": "2"}, {"ACE355_SAMPLE_GRAPH": "1", "ACE355_DUAL": "0"},
            {"ACE355_MX_CROSS": "1", "ACE355_MX_MASK": "61"}]   # (61: every projection but o_proj)
TINY = dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, head_dim=128)
MID = dict(hidden_size=1024, intermediate_size=3072, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=4)
WIDE = dict(hidden_size=2048, intermediate_size=6144, num_hidden_layers=2, num_attention_heads=16, num_key_value_heads=8)


def child(root):
    sys.path.insert(0, root)
    import torch
    import ace355
    from ace355 import weightgen
    from ace355.dit import NativeDit, generate_latents

    def sha(t):
        return hashlib.sha256(t.contiguous().cpu().view(torch.int32).numpy().tobytes()).hexdigest()

    def rnd(seed, *shape):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))

    def make(kw, seed):
        cfg = ace355.DitConfig(**kw)
        dit = NativeDit(cfg, "cuda:0")
        dit.load_state_dict(weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=seed, mode="test"))
        return cfg, dit, weightgen.make_null_condition_emb(cfg.hidden_size, seed=seed)

    def ctx_of(seed, B, T):
        return torch.cat([0.5 * rnd(seed, B, T, 64), torch.ones(B, T, 64)], -1)

    cfg, dit, null = make(TINY, 11)
    B, T, L = 2, 37, 5
    enc, ctx, x = rnd(1, B, L, cfg.hidden_size), ctx_of(2, B, T), rnd(3, B, T, 64)
    dit.set_condition(0, enc[0])
    dit.set_condition(1, enc[1])
    t = [0.7, 0.3]
    print(f"tiny forward {sha(dit.forward(x, ctx, t, t, [0, 1]))}")
    print(f"tiny maps both layers {sha(dit.cross_attention_maps(x, ctx, t, t, [0, 1], [(0, 1), (1, 0), (1, 1)]))}")
    print(f"tiny maps layer 0 {sha(dit.cross_attention_maps(x, ctx, t, t, [0, 1], [(0, 0)]))}")
    kw = dict(seed=[5, 6], infer_steps=4, diffusion_guidance_sale=7.0)
    print(f"tiny sampler cfg {sha(generate_latents(dit, null, enc, ctx, **kw)['target_latents'])}")
    print(f"tiny sampler cfg again {sha(generate_latents(dit, null, enc, ctx, **kw)['target_latents'])}")
    print(f"tiny sampler cover switch {sha(generate_latents(dit, null, enc, ctx, audio_cover_strength=0.5, encoder_hidden_states_non_cover=rnd(4, B, L + 4, cfg.hidden_size), context_latents_non_cover=ctx_of(5, B, T), **kw)['target_latents'])}")
    print(f"tiny sampler sde {sha(generate_latents(dit, null, enc, ctx, infer_method='sde', sde_noise=rnd(6, 4, B, T, 64), **kw)['target_latents'])}")
    print(f"tiny sampler no cfg {sha(generate_latents(dit, null, enc, ctx, seed=[5, 6], infer_steps=4, diffusion_guidance_sale=1.0)['target_latents'])}")
    print(f"tiny dedup forwards {dit.dedup_count()} dual calls {dit.dual_count()}")
    dit.close()

    cfg, dit, null = make(MID, 3)
    enc, ctx = rnd(7, 1, 33, cfg.hidden_size), ctx_of(8, 1, 200)
    print(f"mid sampler cfg {sha(generate_latents(dit, null, enc, ctx, seed=[7], infer_steps=4, diffusion_guidance_sale=7.0)['target_latents'])}")
    enc2, ctx2 = rnd(9, 2, 33, cfg.hidden_size), ctx_of(10, 2, 200)
    print(f"mid sampler cfg two songs {sha(generate_latents(dit, null, enc2, ctx2, seed=[7, 8], infer_steps=3, diffusion_guidance_sale=7.0)['target_latents'])}")
    print(f"mid dual calls {dit.dual_count()}")
    dit.close()

    cfg, dit, null = make(WIDE, 4)
    dit.set_precision("mxfp8")
    B, T, L = 4, 768, 40
    enc, ctx, x = rnd(11, B, L, cfg.hidden_size), ctx_of(12, B, T), rnd(13, B, T, 64)
    for b in range(B):
        dit.set_condition(b, enc[b])
    t = [0.9, 0.6, 0.4, 0.1]
    print(f"wide mxfp8 forward {sha(dit.forward(x, ctx, t, t, [0, 1, 2, 3]))}")
    print(f"wide mxfp8 sampler no cfg {sha(generate_latents(dit, null, enc, ctx, seed=[1, 2, 3, 4], infer_steps=2, diffusion_guidance_sale=1.0)['target_latents'])}")
    dit.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.root)
    lines = []
    for env in SETTINGS:
        tag = " ".join(f"{k}={v}" for k, v in env.items()) or "defaults"
        clean = {k: v for k, v in os.environ.items() if not k.startswith("ACE355_")}
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", args.root], env={**clean, **env}, capture_output=True,
                           text=True, timeout=600)
        if r.returncode != 0:
            sys.exit(f"[{tag}] failed with status {r.returncode}:\n{r.stderr[-4000:]}")
        for ln in r.stdout.splitlines():
            print(f"[{tag}] {ln}", flush=True)
            lines.append(f"[{tag}] {ln}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
