// lm_gqa4_plan_sweep.cpp - stand-alone sweep over csrc/encoder_plan.h (a pure header: no HIP, no library) for causal stacks with FOUR q
// heads per kv head (Qwen3-4B's 32 / 8 layout), the rows tests/encoder_plan_sweep.cpp skips.  Built by tests/test_lm_gqa4_cpu.py with
// the host compiler under -fsanitize=address,undefined.  Every configuration x N x S x cache state below; checks what the executor
// (encoder.hip run_encoder_pass), the allocator (ensure_workspace) and the two causal kernels' launchers rely on:
//   1. every row step carries Hq = 4 Hkv, the QKV row layout [QD | KVD | KVD] and o_ld = QD, with QD = Hq * 128 beside hidden D
//   2. every extent a step reads or writes lies inside plan_encoder_workspace's counts for that request (ao and the QKV rows are
//      QD = 4 KVD wide, wider than D at the 4B's shape)
//   3. a decode step carries plan_lm_decode(pos0 + 1) - a function of the length alone, whatever the ratio -, writes Hq * 128 per
//      sequence, and its partials [seqs][Hq][LM_MAX_SPLITS] fit what lm.hip allocates for max_seqs sequences of Hq heads
//   4. the causal prefill's grid (S / 64 blocks, Hq / 2 head pairs, N) stays inside the launch limits the plan checks
//   5. launcher calls per kind and GEMM FLOPs equal the closed forms; two calls give equal plans
//   6. a 2 : 1 request with the same kv heads gets the same steps in the same order, field for field, except Hq and the widths that follow
//      from QD
// and that every ratio outside {2, 4} is refused by the plan itself, with its text.
#include <stdio.h>
#include <string.h>

#include "../ace-step-1.5-for-windows_amd/csrc/encoder_plan.h"

using namespace ace355;

static long g_fail = 0;
#define EXPECT(cond, ...)                                          \
    do {                                                           \
        if (!(cond)) {                                             \
            if (++g_fail <= 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                          \
    } while (0)

static long g_plans = 0, g_steps = 0, g_refused = 0;
static const char* const RATIO_TEXT = "causal attention: 2 or 4 q heads per kv head";

static void check_pass(const EncPassRequest& r, const char* what) {
    EncPassPlan p = plan_encoder_pass(r);
    EXPECT(!p.error, "refused with '%s' (%s)", p.error ? p.error : "", what);
    if (p.error) return;
    ++g_plans; g_steps += (long)p.steps.size();
    const ace355_encoder_pass_info& f = p.info;
    const long N = r.N, S = r.S, M = N * S, D = r.hidden_size, F = r.intermediate_size, HQ = r.num_heads, KVH = r.num_kv_heads;
    const long QD = HQ * 128, KVD = KVH * 128, QKV = QD + 2 * KVD, NL = r.num_layers;
    const bool cached = r.has_cache, decode = cached && r.pos0 > 0;
    EXPECT(HQ == 4 * KVH && QD == 4 * KVD && QKV == 6 * KVD, "the sweep's own layout (%s)", what);
    const EncWorkspacePlan w = plan_encoder_workspace(&r, 1, 0, 0);
    EXPECT(f.M == M && f.QKV == QKV && f.n_steps == (int)p.steps.size(), "facts (%s)", what);
    EXPECT(w.h == (size_t)(M * D) && w.xn == (size_t)(M * D) && w.qkv == (size_t)((M + ENC_QKV_PAD_ROWS) * QKV) && w.ao == (size_t)(M * QD) &&
               w.act == (size_t)(M * F) && w.vt == 0 && w.vmean == 0, "row buffers (%s)", what);
    EXPECT(f.rope_rows >= (cached ? r.pos0 : 0) + S && (long)w.rope >= f.rope_rows, "rope rows (%s)", what);
    auto size_of = [&](int b) -> size_t {
        switch (b) {
        case ACE355_ENC_BUF_H: return w.h;
        case ACE355_ENC_BUF_XN: return w.xn;
        case ACE355_ENC_BUF_QKV: return w.qkv;
        case ACE355_ENC_BUF_AO: return w.ao;
        case ACE355_ENC_BUF_ACT: return w.act;
        case ACE355_ENC_BUF_OUT: return (size_t)(M * D);   // the caller's
        default: return 0;
        }
    };
    auto inside = [&](const EncStep& s, int b, long elems, size_t i) {
        EXPECT(elems > 0 && (size_t)elems <= size_of(b), "step %zu (kind %d) touches %ld elements of buffer %d, %zu held (%s)", i, s.kind, elems, b, size_of(b), what);
    };
    int calls[ACE355_ENC_STEP_KINDS] = {};
    double flops = 0;
    int stored_layer = -1;
    for (size_t i = 0; i < p.steps.size(); ++i) {
        const EncStep& s = p.steps[i];
        EXPECT(s.kind >= 0 && s.kind < ACE355_ENC_STEP_KINDS && s.layer >= -1 && s.layer < NL, "kind / layer (%s)", what);
        if (s.kind < 0 || s.kind >= ACE355_ENC_STEP_KINDS) continue;
        calls[s.kind]++;
        const bool row_step = s.kind != ACE355_ENC_STEP_RMSNORM && s.kind != ACE355_ENC_STEP_GEMM;
        if (row_step)   // 1.
            EXPECT(s.src == ACE355_ENC_BUF_QKV && s.seqs == N && s.Sq == S && s.Hq == HQ && s.Hkv == KVH && s.Hq == 4 * s.Hkv && s.ld == QKV && s.k_col0 == QD &&
                       s.v_col0 == QD + KVD && s.o_ld == QD && s.layer >= 0, "a QKV row step's shape (%s)", what);
        switch (s.kind) {
        case ACE355_ENC_STEP_RMSNORM:
            EXPECT(s.src == ACE355_ENC_BUF_H && s.M == M && s.N == D, "norm (%s)", what);
            inside(s, s.src, (long)s.M * s.N, i);
            inside(s, s.dst, (long)s.M * s.N, i);
            break;
        case ACE355_ENC_STEP_GEMM: {
            EXPECT(s.M == M && s.lda == s.K && s.ldw == s.K && s.K % 64 == 0 && s.flops == 2.0 * s.M * s.N * (double)s.K, "GEMM numbers (%s)", what);
            const long want_n = s.proj == ACE355_ENC_PROJ_QKV ? QKV : s.proj == ACE355_ENC_PROJ_GATE_UP ? 2 * F : D;
            const long want_k = s.proj == ACE355_ENC_PROJ_O ? QD : s.proj == ACE355_ENC_PROJ_DOWN ? F : D;
            EXPECT(s.N == want_n && s.K == want_k, "projection %d is %d x %d, wanted %ld x %ld (%s)", s.proj, s.N, s.K, want_n, want_k, what);
            if (s.mode == 4) EXPECT(s.hn_q_cols == QD && s.hn_qk_cols == QD + KVD && s.hn_qk_cols <= s.N && s.rope_row0 == (cached ? r.pos0 : 0), "head epilogue (%s)", what);
            flops += s.flops;
            inside(s, s.src, (long)s.M * s.lda, i);
            inside(s, s.dst, (long)s.M * s.ldc, i);
            break;
        }
        case ACE355_ENC_STEP_KV_STORE:
            EXPECT(cached && s.pos0 == r.pos0 && (long)s.pos0 + s.Sq <= r.max_pos && s.seqs <= r.max_seqs, "kv store (%s)", what);
            inside(s, s.src, (long)s.seqs * s.Sq * s.ld, i);
            stored_layer = s.layer;
            break;
        case ACE355_ENC_STEP_DECODE_ATTN: {   // 3.
            const LmDecodePlan d = plan_lm_decode(r.pos0 + 1);
            EXPECT(decode && S == 1 && s.len == r.pos0 + 1 && s.len <= r.max_pos && s.seqs <= r.max_seqs && s.first == 1, "decode attention (%s)", what);
            EXPECT(s.chunk == d.chunk && s.splits == d.splits && s.splits >= 1 && s.splits <= LM_MAX_SPLITS && s.chunk % LM_DECODE_KEY_GROUPS == 0 &&
                       (long)s.splits * s.chunk >= s.len && (long)(s.splits - 1) * s.chunk < s.len, "decode cut %d x %d of %d keys (%s)", s.splits, s.chunk, s.len, what);
            EXPECT(stored_layer == s.layer, "decode attention of layer %d before this step's K / V are stored (%s)", s.layer, what);
            // the partials: the last one written, ((seqs - 1) * Hq + Hq - 1) * LM_MAX_SPLITS + splits - 1, inside max_seqs * Hq * LM_MAX_SPLITS
            EXPECT(((long)(s.seqs - 1) * s.Hq + s.Hq - 1) * LM_MAX_SPLITS + s.splits - 1 < (long)r.max_seqs * HQ * LM_MAX_SPLITS, "partials (%s)", what);
            inside(s, s.src, (long)s.seqs * s.ld, i);
            inside(s, s.dst, (long)s.seqs * s.Hq * 128, i);
            break;
        }
        case ACE355_ENC_STEP_CAUSAL_ATTN:   // 4.
            EXPECT(r.causal && !decode && s.first == (cached && r.has_first), "causal attention (%s)", what);
            EXPECT(s.Hq % 2 == 0 && s.Hq / 2 <= 65535 && s.seqs <= 65535, "causal attention's grid (%s)", what);
            inside(s, s.src, (long)s.seqs * s.Sq * s.ld, i);
            inside(s, s.dst, (long)s.seqs * s.Sq * s.o_ld, i);
            break;
        default:
            EXPECT(false, "a bidirectional step (kind %d) in a causal pass (%s)", s.kind, what);
        }
    }
    // 5.
    const long want[ACE355_ENC_STEP_KINDS] = {2 * NL + 1, 4 * NL, cached ? NL : 0, !decode ? NL : 0, decode ? NL : 0, 0, 0, 0};
    for (int k = 0; k < ACE355_ENC_STEP_KINDS; ++k) EXPECT(calls[k] == want[k] && f.calls[k] == want[k], "calls of kind %d: %d, closed form %ld (%s)", k, calls[k], want[k], what);
    const double want_flops = NL * (2.0 * M * QKV * D + 2.0 * M * D * QD + 2.0 * M * 2 * F * D + 2.0 * M * D * F);
    EXPECT(flops == want_flops && f.gemm_flops == want_flops, "GEMM FLOPs %.0f, closed form %.0f (%s)", flops, want_flops, what);
    const EncPassPlan q = plan_encoder_pass(r);
    EXPECT(!q.error && q.steps.size() == p.steps.size() && memcmp(&q.info, &p.info, sizeof p.info) == 0 &&
               (p.steps.empty() || memcmp(q.steps.data(), p.steps.data(), p.steps.size() * sizeof(EncStep)) == 0), "two calls, two plans (%s)", what);
    // 6. the 2 : 1 stack on the same kv heads: the same walk
    EncPassRequest half = r;
    half.num_heads = 2 * r.num_kv_heads;
    const EncPassPlan h = plan_encoder_pass(half);
    EXPECT(!h.error && h.steps.size() == p.steps.size(), "the 2 : 1 plan has other steps (%s)", what);
    if (!h.error && h.steps.size() == p.steps.size())
        for (size_t i = 0; i < p.steps.size(); ++i) {
            const EncStep &a = p.steps[i], &b = h.steps[i];
            EXPECT(a.kind == b.kind && a.layer == b.layer && a.src == b.src && a.dst == b.dst && a.proj == b.proj && a.norm == b.norm && a.mode == b.mode && a.M == b.M &&
                       a.Hkv == b.Hkv && a.seqs == b.seqs && a.Sq == b.Sq && a.Skv == b.Skv && a.len == b.len && a.chunk == b.chunk && a.splits == b.splits &&
                       a.first == b.first && a.pos0 == b.pos0 && a.rope_row0 == b.rope_row0, "step %zu differs from the 2 : 1 plan's beyond Hq (%s)", i, what);
        }
}

static void expect_refusal(EncPassRequest r, const char* text, const char* what) {
    const EncPassPlan p = plan_encoder_pass(r);
    ++g_refused;
    EXPECT(p.error && strcmp(p.error, text) == 0 && p.steps.empty(), "wanted the refusal '%s', got '%s' (%s)", text, p.error ? p.error : "(a plan)", what);
}

int main() {
    struct Dims { int D, F, HQ, KVH, NL; };
    // the tests' two small stacks, the 4B itself, one kv head, and a stack without layers
    const Dims dims[] = {{256, 768, 8, 2, 2}, {768, 1216, 32, 8, 2}, {2560, 9728, 32, 8, 36}, {256, 512, 4, 1, 3}, {256, 768, 8, 2, 0}};
    const int Ns[] = {1, 2, 3, 16}, Ss[] = {1, 63, 64, 65, 130, 512, 2048};
    char what[256];
    for (const Dims& d : dims) {
        EncPassRequest base{};
        base.hidden_size = d.D; base.intermediate_size = d.F; base.num_heads = d.HQ; base.num_kv_heads = d.KVH; base.num_layers = d.NL;
        for (int N : Ns) {
            for (int S : Ss) {
                EncPassRequest r = base;
                r.causal = 1; r.N = N; r.S = S;
                snprintf(what, sizeof what, "causal D %d NL %d N %d S %d", d.D, d.NL, N, S);
                check_pass(r, what);
            }
            for (int max_seqs : {N, 16}) {
                for (int first = 0; first < 2; ++first)
                    for (int S : Ss)
                        for (int max_pos : {S, S + 7, 4096}) {
                            EncPassRequest r = base;
                            r.causal = 1; r.N = N; r.S = S; r.has_cache = 1; r.pos0 = 0; r.max_pos = max_pos; r.max_seqs = max_seqs; r.has_first = first;
                            snprintf(what, sizeof what, "prefill D %d NL %d N %d S %d max_pos %d first %d", d.D, d.NL, N, S, max_pos, first);
                            check_pass(r, what);
                        }
                for (int len : {2, 64, 65, 255, 256, 257, 258, 1023, 1024, 1025, 1026, 4096, 16384})
                    for (int max_pos : {len, len + 1, 16384}) {
                        EncPassRequest r = base;
                        r.causal = 1; r.N = N; r.S = 1; r.has_cache = 1; r.pos0 = len - 1; r.max_pos = max_pos; r.max_seqs = max_seqs; r.has_first = 1;
                        snprintf(what, sizeof what, "decode D %d NL %d N %d len %d max_pos %d", d.D, d.NL, N, len, max_pos);
                        check_pass(r, what);
                    }
            }
        }
    }
    // ---- the ratios the causal kernels do not serve: refused by the plan, on each causal path; a stack without layers runs no attention
    for (int ratio : {1, 3, 5, 8, 16}) {
        EncPassRequest r{};
        r.hidden_size = 256; r.intermediate_size = 768; r.num_heads = 2 * ratio; r.num_kv_heads = 2; r.num_layers = 2; r.N = 2; r.S = 8; r.causal = 1;
        snprintf(what, sizeof what, "ratio %d", ratio);
        expect_refusal(r, RATIO_TEXT, what);
        EncPassRequest q = r;
        q.has_cache = 1; q.max_pos = 32; q.max_seqs = 2; q.has_first = 1;
        expect_refusal(q, RATIO_TEXT, what);
        q.S = 1; q.pos0 = 8;
        expect_refusal(q, RATIO_TEXT, what);
        q = r; q.causal = 0;   // the bidirectional kernel takes every multiple
        EXPECT(!plan_encoder_pass(q).error, "a bidirectional pass at ratio %d was refused", ratio);
    }
    {
        EncPassRequest r{};
        r.hidden_size = 2560; r.intermediate_size = 9728; r.num_heads = 40; r.num_kv_heads = 8; r.num_layers = 36; r.N = 2; r.S = 512; r.causal = 1;
        expect_refusal(r, RATIO_TEXT, "40 / 8");
        r.num_heads = 32; r.N = 65536; r.S = 1;
        expect_refusal(r, "causal attention: sizes", "the older refusal keeps its place");
    }
    printf("gqa4 pass plans: %ld planned (%ld steps), %ld refused; failures: %ld\n", g_plans, g_steps, g_refused, g_fail);
    return g_fail ? 1 : 0;
}
