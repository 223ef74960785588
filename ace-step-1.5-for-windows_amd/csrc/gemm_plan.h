// gemm_plan.h - the host-side launch decision of gemm.hip as data: what a launch is asked for (GemmRequest), the process's switches
// (GemmKnobs) and what launch_gemm / launch_gemm_mx then do (GemmPlan).  plan_gemm is a pure function of the first two: it reads no
// global, makes no HIP call and allocates nothing, so ace355_gemm_plan can answer for any shape on a machine without a GPU.
#pragma once
#include "common.h"

namespace ace355 {

// Every ACE355_GEMM_* switch and ACE355_MAX_WGS, read once per process (gemm_knobs).  All but krot are A/B and test hooks.
struct GemmKnobs {
    int big;         // ACE355_GEMM_BIG (1): 0 never an 8-wave tile, 1 heuristic, 2 always 192x256, 3 always 192x128 (not SwiGLU)
    int mt1;         // ACE355_GEMM_MT1 (1): 0 no 64-row tiles
    int deep;        // ACE355_GEMM_DEEP (-1): 3-4 stage pipeline of the 4-wave tiles; -1 heuristic (one workgroup per CU), 0 never, 1 always
    int pers;        // ACE355_GEMM_PERS (1): persistent workgroups for multi-round 192x256 launches; 2 also the residual mode; 0 never
    int group_m;     // ACE355_GEMM_GROUPM (4): rasterisation group height inside an XCD region, in tiles
    int xcd_m;       // ACE355_GEMM_XCDM (0): 1 / 2 / 4 / 8 pin the XCD grid's row count (bf16 launches); else by cost
    int mid_ns;      // ACE355_GEMM_MIDNS (3): LDS stages of the 192x128 tile; 2 has no head epilogue
    int krot;        // ACE355_GEMM_KROT (1), ace355_gemm_set_k_rotation: K rotation of 0 no launch (and no split-K), 1 launches with N <= 2048, 2 every launch
    int krot_row;    // ACE355_GEMM_KROT_ROW (1): row stagger of the rotation in K steps, 0 .. 15
    int ksplit;      // ACE355_GEMM_KSPLIT (0): 0 heuristic, n >= 1 that many K parts where split-K applies (1: none)
    int skord;       // ACE355_GEMM_SKORD (1): 0 split-K parts add with fp32 atomics in arrival order even where counters were lent
    int headepi;     // ACE355_GEMM_HEADEPI (1): 0 head-norm + RoPE always as mode 0 + the standalone kernel
    int vt;          // ACE355_GEMM_VT (2): V^T from the head epilogue; 0 never, 1 not on the 192x256 tiles
    int pf;          // ACE355_GEMM_PF (1): 0 no weight-prefetch workgroups anywhere
    int scalar_epi;  // ACE355_GEMM_SCALAR_EPI (0): 1 every bf16 launch takes the scalar epilogue
    int clk;         // ACE355_GEMM_CLK (0): GemmEpilogue::clk_probe (diagnostic; bits 1 / 2 give wrong results)
    int max_wgs;     // ACE355_MAX_WGS (256): the CUs a launch plans for when the caller names none; 8 .. 256, a multiple of 8
};
const GemmKnobs& gemm_knobs();

constexpr int GEMM_PLACEMENT_UNKNOWN = -1, GEMM_PLACEMENT_REFUSED = 0, GEMM_PLACEMENT_VERIFIED = 1;

// What the decision depends on, and nothing else.
struct GemmRequest {
    int M, N, K, mode;   // mode: GemmEpilogue::mode as the caller asks for it
    int fp8;             // MXFP8 operands (launch_gemm_mx); K counts fp8 elements
    int cu_slots;        // GemmEpilogue::cu_slots: 8 .. 256 = plan for that many CUs, else GemmKnobs::max_wgs
    int aligned;         // C, ldc and the per-column vectors allow the 16-byte epilogue (gemm.hip make_request)
    int counters;        // split-K turn counters were lent (GemmEpilogue::sk_cnt)
    int fold_producer, fold_consumer;   // GemmEpilogue::nf_xg / nc_rowsq are set
    int hn_q_cols, hn_qk_cols;          // mode 4: the q | k | v column boundaries
    int vt_offered, vt_heads;           // mode 4: a V^T buffer with a row pitch was offered, and its head count
    int pf_x;            // prefetch workgroups per XCD the caller attached together with a target (gemm_prefetch_plan), 0: none
    int placement;       // GEMM_PLACEMENT_*: the one-time workgroup -> XCD check behind split-K (gemm_verify_splitk_placement)
};

struct GemmPlan {
    // the kernel: gemm_sp_kernel<mode, mt, wnw, ntw, pers, ns, fp8>, a (64 mt) x (32 wnw ntw) tile on 2 wnw waves
    int mode, mt, wnw, ntw, pers, ns, fp8;
    // the launch, and the kernel's tile-map arguments
    int grid_x, grid_y, threads, tiles_n, nwg, group_m, xcd_m;
    // the GemmEpilogue fields the launcher sets (krot carries the row stagger in bits 4 ..)
    int ksplit, kparts, sk_ord, krot, wide_ok, pf_x;
    int head_fused;   // a mode 4 request runs its head epilogue in the GEMM; 0: `mode` is 0 and launch_headnorm_rope2 follows
    int vt_epilogue;  // V^T leaves from the epilogue (GemmEpilogue::vt_out stays set, *vt_done = 1)
};
GemmPlan plan_gemm(const GemmRequest& rq, const GemmKnobs& kn);

// The query behind ace355_gemm_plan (api.hip), not part of a launch: a request (with the process's placement state where asked), its plan
// under the process's knobs, and the XCD column regions gemm_prefetch_plan would hand a PRECEDING launch for it (all zero where it
// attaches none).
struct GemmPrefetchRegions { int pf_x, pf_xcd_n; unsigned pf_chunk16, pf_len16; };
GemmPlan gemm_plan_query(GemmRequest rq, bool process_placement, GemmPrefetchRegions* pf);

}  // namespace ace355
