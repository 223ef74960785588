// attn_plan.h - the host-side launch decision of attn.hip as data, in the shape of gemm_plan.h: what a launch is asked for (AttnRequest),
// the process's switches (AttnKnobs) and what launch_attention then does (AttnPlan).  plan_attention is a pure function of the first
// two: it reads no global, no environment and makes no HIP call, so ace355_attn_plan can answer for any shape on a machine without a GPU.
#pragma once

namespace ace355 {

// Every ACE355_ATTN_* switch and ACE355_MAX_WGS, read once per process (attn_knobs).  All are A/B and test hooks.
struct AttnKnobs {
    int gqa;        // ACE355_ATTN_GQA (-1): 0 attn3_kernel only, 3 / 4 / 6 pin attn_gqa_kernel's NWH wherever Hq == 2 Hkv; else by grid size
    int rot;        // ACE355_ATTN_ROT (1): attn_rot_kernel 0 never, 1 where the 96-row GQA kernel would run, 2 wherever a GQA kernel would
    int nw;         // ACE355_ATTN_NW (0): 4 / 8 pin attn3_kernel's wave count; else by problem size
    int kvsplit;    // ACE355_ATTN_KVSPLIT (0): 0 heuristic, 1 no split-KV, n that many parts wherever the split applies
    float defer;    // ACE355_ATTN_DEFER (8.0): the kernels' deferred-rescale threshold in log2 units; 0 rescales whenever a max moves
    int clk;        // ACE355_ATTN_CLK (0): AttnArgs::clk_probe (diagnostic: bit 0 probe + print, further bits ablations with wrong results)
    int max_wgs;    // ACE355_MAX_WGS (256): the CUs a launch plans for when the caller names none; 8 .. 256
    int one_order;  // no switch of its own: launch_attention sets it per call from K rotation mode 0 (ace355_gemm_set_k_rotation), "one
                    // summation order whatever the launch shape" - no key-split kernel and no split-KV, whose merges are another fp32 order
};
const AttnKnobs& attn_knobs();   // one_order is 0 here

// What the decision depends on, and nothing else.
struct AttnRequest {
    int N, Sq, Skv, Hq, Hkv, window;   // as AttnArgs
    int cu_slots;       // AttnArgs::cu_slots: 8 .. 256 = plan for that many CUs, else AttnKnobs::max_wgs
    int has_kv_len;     // a key-padding mask (AttnArgs::kv_len) is set
    int mx_out;         // MXFP8 output is asked for (AttnArgs::out_q)
    long part_floats;   // the split-KV scratch lent (AttnArgs::part), 0: none
};

constexpr int ATTN_KERNEL_ATTN3 = 0, ATTN_KERNEL_GQA = 1, ATTN_KERNEL_ROT = 2;

struct AttnPlan {
    int kernel, nw;     // ATTN_KERNEL_*: attn3_kernel<nw = 4 | 8>, attn_gqa_kernel<nw = 3 | 4 | 6>, attn_rot_kernel<nw = 3>
    int grid_x, grid_y, grid_z, threads;
    int kv_split;       // AttnArgs::kv_split: workgroups sharing the key tiles of one (q-block, head, sequence); 1 = one pass
    int merge_grid;     // workgroups of the attn_merge_kernel launch that follows, 0: none
    int mx_out_ok;      // this request's kernel can write MXFP8 (a GQA kernel without a key-padding mask), asked for or not
};

inline AttnPlan plan_attention(const AttnRequest& r, const AttnKnobs& kn) {
    AttnPlan p{};
    p.grid_y = p.grid_z = p.kv_split = 1;
    // GQA-shared kernel (Hq = 2 Hkv): one workgroup per (sequence, KV head, 32 NWH query rows), both q heads off one K / V^T tile.  NWH =
    // the largest of {6, 4, 3} whose grid still gives every CU a workgroup; attn3_kernel keeps the small problems and other group sizes.
    auto units = [&](int nwh) { return (long)r.N * r.Hkv * ((r.Sq + 32 * nwh - 1) / (32 * nwh)); };
    const int cus = (r.cu_slots >= 8 && r.cu_slots <= 256) ? r.cu_slots : kn.max_wgs;
    int nwh = 0;
    if (r.Hq == 2 * r.Hkv && kn.gqa != 0) {
        if (kn.gqa == 3 || kn.gqa == 4 || kn.gqa == 6) nwh = kn.gqa;
        else if (units(6) >= 224 * cus / 256) nwh = 6;
        else if (units(4) >= 224 * cus / 256) nwh = 4;
        else if (units(3) >= 128 * cus / 256) nwh = 3;
    }
    p.mx_out_ok = nwh != 0 && !r.has_kv_len;
    if (nwh) {
        // rotated key-split kernel (12 waves per 96-row block) where the 96-row GQA kernel would run: the metric's cross-attention
        const bool rot = !r.mx_out && !kn.one_order && (kn.rot >= 2 || (kn.rot == 1 && nwh == 3));
        p.kernel = rot ? ATTN_KERNEL_ROT : ATTN_KERNEL_GQA;
        p.nw = rot ? 3 : nwh;
        p.grid_x = (int)((units(p.nw) + 7) / 8 * 8);   // 1-D: the kernels decode (q-block, KV head, sequence) XCD-aware
        p.threads = rot ? 768 : 128 * nwh;
        return p;
    }
    // 2 waves per SIMD (256-VGPR budget): 4-wave blocks (128 queries, two workgroups per CU) by default; 8-wave blocks (256 queries, K/V
    // staged once per 256 rows) when the sequence is long enough to fill the chip with them
    const long heads = (long)r.Hq * r.N;
    p.kernel = ATTN_KERNEL_ATTN3;
    p.nw = (kn.nw == 4 || kn.nw == 8) ? kn.nw : (r.Sq >= 1024 && heads * ((r.Sq + 255) / 256) >= 512) ? 8 : 4;
    const int qbk = p.nw * 32, nqb = (r.Sq + qbk - 1) / qbk;
    // split-KV: few workgroups, each with a long serial walk over the 64-key tiles (batch-1 requests) -> up to 8 workgroups per (q-block,
    // head, sequence), at least two tiles each, about one workgroup per CU in total; needs the caller's scratch and no key-padding mask
    // (the all-masked-row rule of the encoders lives in the one-pass epilogue)
    // (measured at batch 1, S = 375: the 13-tile cross-attention walk 22.2 -> 13.9 + 5.2 us in 4 parts; the 6-tile self-attention
    //  14.1 -> 12.9 + 5.1 us in 2 parts, a loss: the fp32 partials and the merge launch cost ~8 us, so only long walks split)
    const long wgs = (long)nqb * heads;
    int tiles = (r.Skv + 63) / 64;
    if (r.window >= 0 && (qbk + 2 * r.window + 63) / 64 + 1 < tiles) tiles = (qbk + 2 * r.window + 63) / 64 + 1;
    if (p.nw == 4 && r.part_floats > 0 && !r.has_kv_len && !r.mx_out && wgs < 128 && tiles >= 8 && !kn.one_order) {
        int sp = 1;
        while (sp < 8 && wgs * sp * 2 <= 256 && tiles / (sp * 2) >= 2) sp *= 2;
        if (kn.kvsplit >= 1) sp = kn.kvsplit;
        if ((long)sp * r.N * r.Hq * r.Sq * 132 <= r.part_floats) p.kv_split = sp;
    }
    p.grid_x = nqb * p.kv_split, p.grid_y = r.Hq, p.grid_z = r.N;
    p.threads = 64 * p.nw;
    if (p.kv_split > 1) p.merge_grid = (int)(((long)r.N * r.Hq * r.Sq + 7) / 8);
    return p;
}

// A request's plan under the process's switches and the K rotation mode of this moment: what launch_attention does, and ace355_attn_plan reports.
AttnPlan attn_plan_query(const AttnRequest& rq);

}  // namespace ace355
