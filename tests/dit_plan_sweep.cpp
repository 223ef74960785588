// dit_plan_sweep.cpp - stand-alone sweep over csrc/dit_plan.h (a pure header: no HIP, no library), built by tests/test_dit_plan_cpu.py with
// the host compiler under -fsanitize=address,undefined.  Random configurations within ace355_dit_create's checks, N 1 .. 64, slot layouts,
// every switch setting; checks what the executor (dit.hip run_pass) relies on:
//   1. every role a step reads was written by an earlier step or is an input, and V^T is fresh for every self-attention
//   2. every row range lies within plan_dit_workspace's / plan_normfold_tables' sizes for that call
//   3. every a_zero_idx points at the zero row (row M of xn / ao / act)
//   4. every fold consumer has its producers: the row sums it reads were added for all of its rows since the zero fill
//   5. the prefetch target of a step is the next projection of the layer loop (the last one wraps to layer 0's QKV with M rows)
//   6. summed FLOPs and the launch count equal the closed-form count
// and the sampler call plan: the split covers the batch, two chains only where the rule allows, the measured policy points.
// Usage: dit_plan_sweep [calls]
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <random>

#include "../ace-step-1.5-for-windows_amd/csrc/dit_plan.h"

using namespace ace355;

static long g_fail = 0;
#define EXPECT(cond, ...)                                          \
    do {                                                           \
        if (!(cond)) {                                             \
            if (++g_fail <= 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                          \
    } while (0)

struct Rows { long lo = 0, hi = 0; };   // rows [lo, hi) of a row-sum vector added since the zero fill
static void cover(Rows& r, long lo, long hi) {
    if (lo >= hi) return;
    if (r.lo == r.hi) { r.lo = lo; r.hi = hi; return; }
    EXPECT(lo <= r.hi && hi >= r.lo, "row sums added in two separate ranges [%ld, %ld) and [%ld, %ld)", r.lo, r.hi, lo, hi);
    r.lo = lo < r.lo ? lo : r.lo;
    r.hi = hi > r.hi ? hi : r.hi;
}

static void check_pass(const DitPassRequest& r, const DitKnobs& kn, long id) {
    const DitPassPlan p = plan_dit_pass(r, kn);
    if (p.error) return;
    const ace355_dit_config& c = r.cfg;
    const ace355_dit_pass_info& f = p.info;
    const int D = c.hidden_size, F = c.intermediate_size, NL = c.num_layers, QD = c.num_heads * 128, KVD = c.num_kv_heads * 128, QKV = QD + 2 * KVD;
    const long M = f.M, S = f.S;
    EXPECT(f.M == r.N * f.S && f.Mc == f.Nc * f.S && f.Nc + f.n_sc == r.N && f.Sp % 64 == 0 && f.Sp >= f.S && f.Sp - f.S < 64, "facts, call %ld", id);
    EXPECT(f.n_steps == (int)p.steps.size(), "n_steps, call %ld", id);
    EXPECT(!f.fold || (r.nf_on && r.temb_rows == 1 && M <= r.nf_cap_M), "fold outside the sampler path, call %ld", id);
    const DitWorkspacePlan w = plan_dit_workspace(c, r.N, r.T);
    const NormfoldTablesPlan t = plan_normfold_tables(c, r.nf_rows > 0 ? r.nf_rows : 1, r.nf_cap_M > 0 ? r.nf_cap_M : 0);
    auto size_of = [&](int role) -> size_t {
        switch (role) {
        case ACE355_DIT_BUF_XIN: return w.xin;
        case ACE355_DIT_BUF_H: return w.h;
        case ACE355_DIT_BUF_XN: return w.xn;
        case ACE355_DIT_BUF_QKV: return w.qkv;
        case ACE355_DIT_BUF_AO: return w.ao;
        case ACE355_DIT_BUF_ACT: return w.act;
        case ACE355_DIT_BUF_AQ: return w.aq;
        case ACE355_DIT_BUF_XQ: return w.xq;
        case ACE355_DIT_BUF_VT: return w.vt;
        case ACE355_DIT_BUF_VPAD: return w.vpad;
        default: return ~(size_t)0;
        }
    };
    EXPECT((size_t)f.vt_elems <= w.vt, "V^T memset beyond the buffer, call %ld", id);
    std::map<int, long> written;   // role -> rows written so far (inputs: the packed patches, the condition slots)
    written[ACE355_DIT_BUF_XIN] = M;
    written[ACE355_DIT_BUF_SLOT_KV] = 1;
    std::map<int, Rows> sums;
    bool vt_fresh = false;
    long launches = 0;
    double gemm_flops = 0, attn_flops = 0;
    auto reads = [&](const DitStep& s, int role, long rows, long ld, size_t i) {
        EXPECT(written.count(role) && written[role] >= rows, "step %zu (kind %d layer %d) reads %ld rows of role %d, %ld written, call %ld", i, s.kind, s.layer, rows,
               role, written.count(role) ? written[role] : -1, id);
        EXPECT((size_t)(rows * ld) <= size_of(role), "step %zu reads beyond role %d, call %ld", i, role, id);
    };
    auto writes = [&](int role, long rows, long ld, size_t i) {
        EXPECT((size_t)(rows * ld) <= size_of(role), "step %zu writes beyond role %d, call %ld", i, role, id);
        written[role] = written[role] > rows ? written[role] : rows;
    };
    for (size_t i = 0; i < p.steps.size(); ++i) {
        const DitStep& s = p.steps[i];
        EXPECT(s.layer >= -1 && s.layer < NL, "layer, call %ld", id);
        switch (s.kind) {
        case ACE355_DIT_STEP_ZERO_ROWSQ:
            EXPECT(f.fold && (size_t)s.count <= t.rowsq && s.count == (long)NL * 3 * M, "row-sum zero fill, call %ld", id);
            sums.clear();
            break;
        case ACE355_DIT_STEP_MOD_GS: EXPECT(!f.emb && s.M == r.temb_rows && (size_t)s.M * NL * 4 * D <= w.gs, "mod_gs, call %ld", id); break;
        case ACE355_DIT_STEP_NORM_GS: case ACE355_DIT_STEP_NORM_GS_MX: case ACE355_DIT_STEP_NORM_W: case ACE355_DIT_STEP_NORM_W_MX: case ACE355_DIT_STEP_NORM_OUT: {
            const bool gs = s.kind == ACE355_DIT_STEP_NORM_GS || s.kind == ACE355_DIT_STEP_NORM_GS_MX;
            EXPECT(!gs || (s.gs >= 0 && s.gs < 2 * NL && s.gs / 2 == s.layer), "(g, shift) entry, call %ld", id);
            EXPECT(!f.fold || s.kind == ACE355_DIT_STEP_NORM_OUT || (s.layer == 0 && s.gs == 0), "a norm kernel in a folded pass, call %ld", id);
            reads(s, s.src, s.M, D, i);
            writes(s.dst, s.M, D, i);
            break;
        }
        case ACE355_DIT_STEP_TRANSPOSE_V:
            reads(s, ACE355_DIT_BUF_QKV, s.seqs * S, QKV, i);
            EXPECT((size_t)s.seqs * c.num_kv_heads * 128 * f.Sp <= w.vt, "transpose_v beyond V^T, call %ld", id);
            vt_fresh = true;
            break;
        case ACE355_DIT_STEP_TAP: reads(s, ACE355_DIT_BUF_H, M, D, i); EXPECT(s.count == M * D && ((r.tap_mask >> s.layer) & 1), "tap, call %ld", id); break;
        case ACE355_DIT_STEP_ATTN_SELF: case ACE355_DIT_STEP_ATTN_CROSS: {
            const bool self = s.kind == ACE355_DIT_STEP_ATTN_SELF;
            reads(s, ACE355_DIT_BUF_QKV, s.seqs * S, self ? QKV : QD, i);
            EXPECT(!self || vt_fresh, "self-attention of layer %d without a fresh V^T, call %ld", s.layer, id);
            if (self) vt_fresh = false;
            EXPECT(s.Sq == S && s.Skv == (self ? S : f.L) && s.seqs == (self ? (f.dedup0 && s.layer == 0 ? f.Nc : r.N) : f.Nc), "attention shape, call %ld", id);
            EXPECT(self || (s.Lpad == f.Lpad && s.window == -1), "cross-attention, call %ld", id);
            writes(s.dst, s.seqs * S, QD, i);
            EXPECT(s.dst == (s.mx_out ? ACE355_DIT_BUF_XQ : ACE355_DIT_BUF_AO), "attention output role, call %ld", id);
            attn_flops += s.flops;
            break;
        }
        case ACE355_DIT_STEP_XATTN_PROBS:
            reads(s, ACE355_DIT_BUF_QKV, s.seqs * S, QD, i);
            EXPECT(s.n_heads == r.map_heads[s.layer] && s.n_heads > 0 && s.seqs == f.Nc, "xattn_probs, call %ld", id);
            break;
        case ACE355_DIT_STEP_GEMM: {
            ++launches;
            gemm_flops += s.flops;
            EXPECT(s.flops == 2.0 * s.M * s.N * (double)s.K && s.ldw == s.K && s.lda == s.K, "GEMM numbers, call %ld", id);
            const long a_rows = s.a_wrap ? s.a_wrap : s.M;
            if (s.path == ACE355_DIT_PATH_MX) EXPECT(s.src == ACE355_DIT_BUF_XQ || s.src == ACE355_DIT_BUF_AQ, "MX operand role, call %ld", id);
            else EXPECT(s.src == ACE355_DIT_BUF_XIN || s.src == ACE355_DIT_BUF_XN || s.src == ACE355_DIT_BUF_AO || s.src == ACE355_DIT_BUF_ACT, "bf16 operand role, call %ld", id);
            reads(s, s.src, a_rows, s.lda, i);
            if (s.path == ACE355_DIT_PATH_MX_QUANT) writes(ACE355_DIT_BUF_XQ, s.M, s.K, i);
            EXPECT(s.path == ACE355_DIT_PATH_BF16 || (r.precision == ACE355_PRECISION_MXFP8 && s.M >= r.mx_min_rows && dit_mx_shape_ok(s.M, s.N, s.K, s.mode)), "MX path, call %ld", id);
            // 3. the zero row
            EXPECT(s.a_zero_idx == 0 || (kn.zrow && s.a_zero_idx == M && s.path == ACE355_DIT_PATH_BF16 &&
                                         (s.src == ACE355_DIT_BUF_XN || s.src == ACE355_DIT_BUF_AO || s.src == ACE355_DIT_BUF_ACT) &&
                                         (size_t)(s.a_zero_idx + 1) * s.lda <= size_of(s.src) && s.a_zero_idx >= s.M), "a_zero_idx %d, call %ld", s.a_zero_idx, id);
            EXPECT(s.a_wrap == 0 || (2 * s.a_wrap >= s.M && f.dedup0 && s.layer == 0 && s.proj == ACE355_DIT_PROJ_O), "a_wrap, call %ld", id);
            writes(s.dst, s.M, s.mode == 3 ? s.N / 2 : s.ldc, i);
            EXPECT(s.mode == 3 ? s.ldc == s.N / 2 : s.ldc == s.N, "ldc, call %ld", id);
            if (s.vt_offered) vt_fresh = i + 1 >= p.steps.size() || p.steps[i + 1].kind != ACE355_DIT_STEP_TRANSPOSE_V;
            // 4. fold
            if (s.nf_split >= 0) {
                EXPECT(f.fold && s.mode == 2 && s.path == ACE355_DIT_PATH_BF16 && s.nf_split <= s.M, "fold producer, call %ld", id);
                for (int idx : {s.nf_sqA, s.nf_sqB}) EXPECT(idx >= 0 && idx < 3 * NL && (size_t)(idx + 1) * M <= t.rowsq, "row-sum index %d, call %ld", idx, id);
                for (int g : {s.nf_gA, s.nf_gB}) EXPECT(g == ACE355_DIT_G_NORM_CA || (g >= 0 && g < 2 * NL), "(g, shift) entry %d, call %ld", g, id);
                cover(sums[s.nf_sqA], 0, s.nf_split);
                cover(sums[s.nf_sqB], s.nf_split, s.M);
                writes(ACE355_DIT_BUF_XN, s.M, D, i);
            }
            if (s.nc_rowsq >= 0) {
                EXPECT(f.fold && s.path == ACE355_DIT_PATH_BF16 && s.src == ACE355_DIT_BUF_XN, "fold consumer, call %ld", id);
                const Rows have = sums.count(s.nc_rowsq) ? sums[s.nc_rowsq] : Rows{};
                EXPECT(have.lo == 0 && have.hi >= s.M, "consumer of row sums %d reads rows [0, %d), produced [%ld, %ld), step %zu, call %ld", s.nc_rowsq, s.M, have.lo, have.hi, i, id);
                EXPECT(s.nc_bias == (s.proj == ACE355_DIT_PROJ_QKV ? 1 : s.proj == ACE355_DIT_PROJ_GATE_UP ? 2 : 0), "consumer bias table, call %ld", id);
                EXPECT(r.nf_rows > 0, "fold without schedule tables, call %ld", id);
            }
            // 5. prefetch
            if (s.next_proj >= 0) {
                EXPECT(r.prefetch && r.precision != ACE355_PRECISION_MXFP8 && s.path == ACE355_DIT_PATH_BF16 && s.layer >= 0, "a target where no prefetch is allowed, call %ld", id);
                const DitStep* nx = nullptr;
                for (size_t j = i + 1; j < p.steps.size() && !nx; ++j)
                    if (p.steps[j].kind == ACE355_DIT_STEP_GEMM && p.steps[j].layer >= 0) nx = &p.steps[j];
                if (nx) EXPECT(nx->proj == s.next_proj && nx->layer == s.next_layer && nx->M == s.next_M && nx->N == s.next_N && nx->K == s.next_K && nx->mode == s.next_mode,
                               "prefetch target of step %zu is not the next projection, call %ld", i, id);
                else if (s.proj == ACE355_DIT_PROJ_DOWN) EXPECT(s.next_proj == ACE355_DIT_PROJ_QKV && s.next_layer == 0 && s.next_M == M && s.next_N == QKV && s.next_K == D && s.next_mode == 4, "the wrap target, call %ld", id);
                else EXPECT(r.map_last == s.layer && s.proj == ACE355_DIT_PROJ_CROSS_Q && s.next_proj == ACE355_DIT_PROJ_CROSS_O, "a target behind the end of the pass, call %ld", id);
            } else {
                EXPECT(!(r.prefetch && r.precision != ACE355_PRECISION_MXFP8 && s.layer >= 0), "a layer projection without its target, call %ld", id);
            }
            break;
        }
        default: EXPECT(false, "unknown step kind %d, call %ld", s.kind, id);
        }
    }
    // 6. closed-form counts
    const bool maps = r.map_last >= 0 && f.Nc > 0 && r.map_heads[r.map_last] > 0;
    const int full_layers = maps ? r.map_last : NL;
    const double Mq0 = f.dedup0 ? f.Mc : M;
    auto layer_gemm = [&](double mq, bool whole) {
        double v = 2.0 * mq * QKV * D + 2.0 * M * D * QD + (f.Nc > 0 ? 2.0 * f.Mc * QD * D : 0);
        if (whole) v += (f.Nc > 0 ? 2.0 * f.Mc * D * QD : 0) + 2.0 * M * (2.0 * F) * D + 2.0 * M * D * F;
        return v;
    };
    double want = 2.0 * M * D * (2.0 * c.in_channels);
    for (int l = 0; l < full_layers; ++l) want += layer_gemm(l == 0 ? Mq0 : M, true);
    if (maps) want += layer_gemm(r.map_last == 0 ? Mq0 : M, false);
    else want += 2.0 * M * (2.0 * c.out_channels) * D;
    const long per_layer = f.Nc > 0 ? 6 : 4;
    const long want_launches = 1 + per_layer * full_layers + (maps ? 3 : 1);
    EXPECT(gemm_flops == want && f.gemm_flops == want, "GEMM FLOPs %.0f, closed form %.0f, call %ld", gemm_flops, want, id);
    EXPECT(launches == want_launches && f.gemm_launches == want_launches, "GEMM launches %ld, closed form %ld, call %ld", launches, want_launches, id);
    double want_attn = 0;
    for (int l = 0; l < (maps ? r.map_last : NL); ++l) {
        const int win = ((c.sliding_layer_mask >> l) & 1ull) ? c.sliding_window : -1;
        want_attn += 4.0 * (l == 0 && f.dedup0 ? f.Nc : r.N) * c.num_heads * (double)S * (win >= 0 ? dit_band_keys(f.S, win) : (double)S) * 128.0;
        if (f.Nc > 0) want_attn += 4.0 * f.Nc * c.num_heads * (double)S * f.L * 128.0;
    }
    if (maps) {
        const int l = r.map_last, win = ((c.sliding_layer_mask >> l) & 1ull) ? c.sliding_window : -1;
        want_attn += 4.0 * (l == 0 && f.dedup0 ? f.Nc : r.N) * c.num_heads * (double)S * (win >= 0 ? dit_band_keys(f.S, win) : (double)S) * 128.0;
    }
    EXPECT(attn_flops == f.attn_flops && (want_attn == 0 ? attn_flops == 0 : attn_flops / want_attn > 1 - 1e-12 && attn_flops / want_attn < 1 + 1e-12), "attention FLOPs %.0f, closed form %.0f, call %ld",
           attn_flops, want_attn, id);
}

static void check_sampler(std::mt19937& rng) {
    long calls = 0;
    for (int B = 1; B <= 32; ++B)
        for (int copies = 1; copies <= 2; ++copies)
            for (int S : {1, 19, 100, 375, 1500, 3000})
                for (int bits = 0; bits < 256; ++bits) {
                    SamplerCallRequest r{B, copies, S, bits & 3, (bits & 4) ? 2400 : (int)(rng() % 5000), (bits & 8) ? 1 << 30 : (int)(rng() % 4000), (bits >> 4) & 1,
                                         (bits >> 5) & 1, (bits >> 6) & 1, (int)(rng() % 2), (bits >> 7) & 1, -1};
                    if (r.dual_mode == 3) continue;
                    const SamplerCallPlan first = plan_sampler_call(r);
                    EXPECT(first.nchains == 1 && first.B0 == B && first.B1 == 0, "two chains before the probe answered");
                    for (int probe = 0; probe <= 1; ++probe) {
                        r.probe = probe;
                        const SamplerCallPlan p = plan_sampler_call(r);
                        ++calls;
                        EXPECT(p.B0 + p.B1 == B && p.B0 >= p.B1 && p.B0 - p.B1 <= 1 + (p.nchains == 1 ? B : 0), "the split covers the batch");
                        EXPECT(!p.needs_probe && p.graph == first.graph && p.under_filled == first.under_filled, "probe answered");
                        EXPECT(p.graph == (r.graph_mode && !r.timing && !r.profile && !r.taps), "graph eligibility");
                        const bool want = r.dual_mode && B >= 2 && !r.taps && r.side_stream && (r.dual_mode >= 2 || (p.under_filled && !p.graph));
                        EXPECT((p.nchains == 2) == (want && probe) && first.needs_probe == want, "chain count");
                        for (int k = 0; k < 2; ++k)
                            EXPECT(p.cu_slots[k] == ((p.nchains == 2 && (k ? p.B1 : p.B0) * copies * S >= r.slots_min_rows) ? 128 : 0), "cu_slots");
                    }
                }
    // the measured policy points (30 s songs with CFG: 750 rows per song): songs -> two chains by default?
    const int two[] = {0, 0, 1, 1, 0, 1, 1, 0, 0, 1, 1};   // index = songs
    for (int songs = 1; songs <= 10; ++songs) {
        const SamplerCallPlan p = plan_sampler_call(SamplerCallRequest{songs, 2, 375, 1, 2400, 1 << 30, 0, 0, 0, 0, 1, 1});
        EXPECT((p.nchains == 2) == (two[songs] != 0), "%d songs: %d chains", songs, p.nchains);
    }
    printf("sampler call plans: %ld\n", calls);
}

int main(int argc, char** argv) {
    const long calls = argc > 1 ? atol(argv[1]) : 20000;
    std::mt19937 rng(12345);
    auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    long planned = 0, refused = 0, steps = 0;
    for (long id = 0; id < calls; ++id) {
        DitPassRequest r{};
        ace355_dit_config& c = r.cfg;
        const bool big = id % 7 == 0;   // the full-size widths, where the MXFP8 forms apply
        c.num_kv_heads = big ? 8 : pick(1, 4);
        c.num_heads = c.num_kv_heads * (big ? 2 : pick(1, 3));
        c.hidden_size = big ? 2048 : 64 * pick(1, 40);
        c.intermediate_size = big ? 6144 : 64 * pick(1, 100);
        c.num_layers = id % 11 == 0 ? pick(24, 64) : pick(1, 5);
        c.head_dim = 128; c.patch_size = 2; c.in_channels = 192; c.out_channels = 64;   // (the packed patch input is laid out for 192 channels: plan_dit_workspace)
        c.sliding_window = pick(0, 200);
        c.sliding_layer_mask = ((uint64_t)rng() << 32) | rng();
        c.rms_norm_eps = 1e-6f; c.rope_theta = 1e6f;
        r.N = id % 5 == 0 ? pick(1, 64) : pick(1, 8);
        r.T = id % 13 == 0 ? pick(1, 3000) : pick(1, 400);
        r.temb_rows = pick(0, 1) ? 1 : r.N;
        const int style = pick(0, 4), L = pick(1, 900);
        for (int i = 0; i < r.N; ++i) {
            // 0: CFG halves (conditions, then one broadcast null slot)  1: all conditions  2: all on one broadcast slot  3: random  4: L mismatch / unset
            const bool null_half = style == 0 && r.N % 2 == 0 && i >= r.N / 2;
            r.seq_slot[i] = null_half || style == 2 ? 31 : style == 3 ? pick(0, 31) : i % 31;
            r.seq_broadcast[i] = null_half || style == 2 || (style == 3 && pick(0, 1));
            r.seq_L[i] = style == 4 ? pick(0, 3) : null_half ? pick(1, 900) : L;
        }
        r.precision = pick(0, 3) == 0 ? ACE355_PRECISION_MXFP8 : ACE355_PRECISION_BF16;
        r.mx_min_rows = pick(0, 1) ? 1536 : pick(1, 2000);
        r.mx_copies = pick(0, 1) ? dit_mx_copies(c) : (dit_mx_copies(c) & pick(0, 63));
        r.nf_on = pick(0, 1); r.nf_emb_on = r.nf_on || pick(0, 1); r.nf_rows = r.nf_emb_on ? pick(1, 60) : 0;
        r.nf_cap_M = pick(0, 3) ? (long)r.N * ((r.T + 1) / 2) + pick(0, 100) : pick(0, 500);
        // (the handle folds only what normfold_eligible allows: no MXFP8 rows, whole 256-column tiles)
        if (r.precision == ACE355_PRECISION_MXFP8 && (long)r.N * ((r.T + 1) / 2) >= r.mx_min_rows) r.nf_on = 0;
        r.dup_half = pick(0, 1); r.dedup_on = pick(0, 3) != 0; r.prefetch = pick(0, 1);
        r.cu_slots = pick(0, 1) ? 0 : 128; r.graph_mode = pick(0, 1);
        r.zr_M = pick(0, 1) ? r.N * ((r.T + 1) / 2) : -1;
        r.tap_mask = pick(0, 3) == 0 ? (((uint64_t)rng() << 32) | rng()) & (c.num_layers == 64 ? ~0ull : (1ull << c.num_layers) - 1) : 0;
        r.map_last = -1;
        if (pick(0, 5) == 0) {
            for (int l = 0; l < c.num_layers; ++l) r.map_heads[l] = pick(0, 2) ? 0 : pick(1, c.num_heads);
            for (int l = 0; l < c.num_layers; ++l) if (r.map_heads[l]) r.map_last = l;
        }
        r.qkv_vt_epilogue = pick(0, 1); r.qkv_vt_epilogue_half = pick(0, 1); r.self_mx_out_ok = pick(0, 1); r.cross_mx_out_ok = pick(0, 1);
        for (int k = 0; k < 16; ++k) {   // every switch setting (the mask: all, none, two subsets)
            const DitKnobs kn{k & 1, (k & 2) ? 63 : (k & 4) ? 61 : (int)(id % 64), (k >> 2) & 1, (k >> 3) & 1};
            const DitPassPlan p = plan_dit_pass(r, kn);
            if (p.error) { ++refused; EXPECT(p.steps.empty(), "a refusal with steps"); continue; }
            ++planned; steps += (long)p.steps.size();
            check_pass(r, kn, id);
        }
    }
    check_sampler(rng);
    printf("pass plans: %ld planned (%ld steps), %ld refused; failures: %ld\n", planned, steps, refused, g_fail);
    return g_fail ? 1 : 0;
}
