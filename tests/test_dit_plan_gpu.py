"""GPU: the handle launches what its pass plan says.  Under profiling a handle counts every GEMM launch and the FLOPs of every GEMM and
attention launch it makes; after a plain forward, one sampler step and a maps call the counts equal the sums over the steps of
native.dit_pass_plan for the same request, exactly."""
import pytest
import torch

from test_dit_gpu import TINY, _make

pytestmark = pytest.mark.gpu

MID = dict(hidden_size=1024, intermediate_size=3072, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=4)   # test_zero_row_and_tile64_switches_keep_the_bits
T, L = 37, 5   # odd T: S = 19; two songs with CFG: 4 x 19 = 76 rows


def _sums(plan):
    n, g, a = 0, 0.0, 0.0
    for st in plan["steps"]:   # (in launch order, as the handle adds them up)
        if st["kind"] == "gemm":
            n, g = n + 1, g + st["flops"]
        elif st["kind"] in ("attn_self", "attn_cross"):
            a += st["flops"]
    assert (n, g, a) == (plan["gemm_launches"], plan["gemm_flops"], plan["attn_flops"])
    return n, g, a


def _profiled(dit, call):
    dit.set_profile(True)
    try:
        call()
        p = dit.get_profile()
    finally:
        dit.set_profile(False)
    return int(p["gemm_launches"]), p["gemm_flops"], p["attn_flops"]


@pytest.mark.parametrize("name,kw,fold", [("tiny", TINY, 0), ("mid", MID, 2)])
def test_profile_counts_equal_the_plans_sums(gpu_device, name, kw, fold):
    from ace355 import native, weightgen
    cfg, _w, dit = _make(kw, 7, gpu_device)
    g = torch.Generator().manual_seed(1)
    enc = torch.randn(2, L, cfg.hidden_size, generator=g)
    ctx = torch.cat([0.5 * torch.randn(2, T, 64, generator=g), torch.ones(2, T, 64)], -1)
    x = torch.randn(2, T, 64, generator=g)
    dit.set_condition(0, enc[0])
    dit.set_condition(1, enc[1])
    dit.set_condition(2, weightgen.make_null_condition_emb(cfg.hidden_size, seed=7).reshape(1, -1), L=L)   # the broadcast null slot
    dit.set_norm_fold(fold)   # 0: norms as kernels; 2: folded wherever the kernels allow (76 rows >= 64)
    dit.set_dual(0)           # one chain: one plan (two chains run one plan each, on their halves)
    cfg_seqs = [(0, L, 0), (1, L, 0), (2, L, 1), (2, L, 1)]
    # (a) plain forward: two songs with their CFG copies on the null slot, one timestep row per sequence
    t = [0.8, 0.8, 0.8, 0.8]
    got = _profiled(dit, lambda: dit.forward(torch.cat([x, x]), torch.cat([ctx, ctx]), t, t, [0, 1, 2, 2]))
    want = _sums(native.dit_pass_plan(cfg, T, cfg_seqs))
    print(f"{name} forward: handle {got}, plan {want}")
    assert got == want
    # (b) one sampler step.  The call before profiling builds the schedule tables (their GEMMs are not the pass's); the profiled call reuses them
    ts = torch.tensor([1.0, 0.5])
    step = lambda: dit.sample(x, ctx, ts, guidance_scale=7.0, cond_slots=[0, 1], null_slot=2)
    step()
    got = _profiled(dit, step)
    plan = native.dit_pass_plan(cfg, T, cfg_seqs, temb_rows=1, dup_half=1, nf_on=int(fold == 2), nf_emb_on=1, nf_rows=1, nf_cap_M=4 * 19)
    assert plan["fold"] == int(fold == 2) and plan["dedup0"] == 1 and plan["n_sc"] == 2
    want = _sums(plan)
    print(f"{name} sampler step: handle {got}, plan {want}")
    assert got == want
    # (c) a maps call that stops at layer 0
    t2 = [0.8, 0.8]
    got = _profiled(dit, lambda: dit.cross_attention_maps(x, ctx, t2, t2, [0, 1], [(0, 0)]))
    plan = native.dit_pass_plan(cfg, T, [(0, L, 0), (1, L, 0)], map_last=0, map_heads=[1, 0])
    assert plan["steps"][-1]["kind"] == "xattn_probs" and plan["gemm_launches"] == 4
    want = _sums(plan)
    print(f"{name} maps: handle {got}, plan {want}")
    assert got == want
    dit.close()
