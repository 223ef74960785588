// encoder_plan_sweep.cpp - stand-alone sweep over csrc/encoder_plan.h (a pure header: no HIP, no library), built by
// tests/test_encoder_plan_cpu.py with the host compiler under -fsanitize=address,undefined.  Every configuration x N x S x cache state below,
// on the three attention paths; checks what the executor (encoder.hip run_encoder_pass) and the allocator (ensure_workspace) rely on:
//   1. every extent a step reads or writes lies inside plan_encoder_workspace's counts for that request - the rows behind M that the
//      attention's last key tile touches in qkv included, and V^T = N * KVH * 128 * Sp
//   2. the rope tables cover pos0 + S, and every cache access lies inside [0, max_pos) x [0, max_seqs)
//   3. a decode step carries plan_lm_decode(pos0 + 1), with splits <= LM_MAX_SPLITS and the chunks covering the keys
//   4. every buffer a step reads was written by an earlier step or is the pass's input
//   5. the window of an attention step is its layer's
//   6. launcher calls per kind and GEMM FLOPs equal the closed forms
//   7. two calls give equal plans, and planning again into the same plan does not reallocate
// and the refusals' texts.
#include <stdio.h>
#include <string.h>

#include <set>

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

static void check_pass(const EncPassRequest& r, const char* what) {
    EncPassPlan p = plan_encoder_pass(r);
    if (p.error) { ++g_refused; EXPECT(p.steps.empty(), "a refusal with steps (%s)", what); return; }
    ++g_plans; g_steps += (long)p.steps.size();
    const ace355_encoder_pass_info& f = p.info;
    const long N = r.N, S = r.S, M = N * S, D = r.hidden_size, F = r.intermediate_size, QD = r.num_heads * 128L, KVD = r.num_kv_heads * 128L, QKV = QD + 2 * KVD;
    const long NL = r.num_layers;
    const bool cached = r.has_cache, decode = cached && r.pos0 > 0;
    const EncWorkspacePlan w = plan_encoder_workspace(&r, 1, 0, 0);
    EXPECT(f.M == M && f.Sp % 64 == 0 && f.Sp >= S && f.Sp - S < 64 && f.QKV == QKV && f.n_steps == (int)p.steps.size(), "facts (%s)", what);
    EXPECT(w.h == (size_t)(M * D) && w.xn == (size_t)(M * D) && w.qkv == (size_t)((M + 64) * QKV) && w.ao == (size_t)(M * QD) && w.act == (size_t)(M * F),
           "row buffers (%s)", what);
    EXPECT(w.vt == (r.causal ? 0 : (size_t)(N * r.num_kv_heads * 128 * f.Sp)), "V^T elements (%s)", what);
    EXPECT(w.vmean == (!r.causal && r.has_kv_len ? (size_t)(N * KVD) : 0) && w.kvlen == (!r.causal && r.has_kv_len ? (size_t)N : 0), "vmean / kvlen (%s)", what);
    // 2. rope
    EXPECT(f.rope_rows >= (cached ? r.pos0 : 0) + S && w.need.rope_rows == f.rope_rows && (long)w.rope >= f.rope_rows && w.rope >= 512 &&
               (w.rope & (w.rope - 1)) == 0 && (w.rope == 512 || (long)w.rope / 2 < f.rope_rows), "rope rows %d, capacity %zu (%s)", f.rope_rows, w.rope, what);
    auto size_of = [&](int b) -> size_t {
        switch (b) {
        case ACE355_ENC_BUF_H: return w.h;
        case ACE355_ENC_BUF_XN: return w.xn;
        case ACE355_ENC_BUF_QKV: return w.qkv;
        case ACE355_ENC_BUF_AO: return w.ao;
        case ACE355_ENC_BUF_ACT: return w.act;
        case ACE355_ENC_BUF_VT: return w.vt;
        case ACE355_ENC_BUF_VMEAN: return w.vmean;
        case ACE355_ENC_BUF_OUT: return (size_t)(M * D);   // the caller's
        default: return 0;
        }
    };
    std::set<int> written{ACE355_ENC_BUF_H};
    int calls[ACE355_ENC_STEP_KINDS] = {};
    double flops = 0;
    auto reads = [&](const EncStep& s, int b, long elems, size_t i) {
        EXPECT(written.count(b), "step %zu (kind %d layer %d) reads buffer %d before anything wrote it (%s)", i, s.kind, s.layer, b, what);
        EXPECT(elems >= 0 && (size_t)elems <= size_of(b), "step %zu (kind %d) reads %ld elements of buffer %d, %zu held (%s)", i, s.kind, elems, b, size_of(b), what);
    };
    auto writes = [&](const EncStep& s, int b, long elems, size_t i) {
        EXPECT(elems > 0 && (size_t)elems <= size_of(b), "step %zu (kind %d) writes %ld elements of buffer %d, %zu held (%s)", i, s.kind, elems, b, size_of(b), what);
        written.insert(b);
    };
    int stored_layer = -1;   // the layer whose K / V this call has stored
    for (size_t i = 0; i < p.steps.size(); ++i) {
        const EncStep& s = p.steps[i];
        EXPECT(s.kind >= 0 && s.kind < ACE355_ENC_STEP_KINDS && s.layer >= -1 && s.layer < NL, "kind / layer (%s)", what);
        if (s.kind < 0 || s.kind >= ACE355_ENC_STEP_KINDS) continue;
        calls[s.kind]++;
        const bool row_step = s.kind != ACE355_ENC_STEP_RMSNORM && s.kind != ACE355_ENC_STEP_GEMM;
        if (row_step)
            EXPECT(s.src == ACE355_ENC_BUF_QKV && s.seqs == N && s.Sq == S && s.Hq == r.num_heads && s.Hkv == r.num_kv_heads && s.ld == QKV && s.k_col0 == QD &&
                       s.v_col0 == QD + KVD && s.o_ld == QD && s.layer >= 0, "a QKV row step's shape (%s)", what);
        switch (s.kind) {
        case ACE355_ENC_STEP_RMSNORM:
            EXPECT(s.src == ACE355_ENC_BUF_H && s.M == M && s.N == D && s.rows_per_seq == S && s.norm == (s.layer < 0 ? 2 : s.norm) && s.norm >= 0 && s.norm <= 2, "norm (%s)", what);
            EXPECT((s.layer < 0) == (s.dst == ACE355_ENC_BUF_OUT) && (s.layer < 0) == (i + 1 == p.steps.size()), "the final norm is the last step (%s)", what);
            reads(s, s.src, (long)s.M * s.N, i);
            writes(s, s.dst, (long)s.M * s.N, i);
            break;
        case ACE355_ENC_STEP_GEMM:
            EXPECT(s.M == M && s.lda == s.K && s.ldw == s.K && s.K % 64 == 0 && s.flops == 2.0 * s.M * s.N * (double)s.K && s.proj >= 0 && s.proj <= 3, "GEMM numbers (%s)", what);
            EXPECT(s.mode == (s.proj == ACE355_ENC_PROJ_QKV ? 4 : s.proj == ACE355_ENC_PROJ_GATE_UP ? 3 : 2) && s.sk_cnt == (s.mode == 2) &&
                       s.rows_per_seq == (s.mode == 3 ? 0 : S), "GEMM mode (%s)", what);
            EXPECT(s.ldc == (s.mode == 3 ? s.N / 2 : s.N), "ldc (%s)", what);
            if (s.mode == 4) {
                EXPECT(s.hn_q_cols == QD && s.hn_qk_cols == QD + KVD && s.hn_qk_cols <= s.N && s.rope_row0 == (cached ? r.pos0 : 0), "head epilogue (%s)", what);
                EXPECT((long)s.rope_row0 + s.rows_per_seq <= f.rope_rows && (long)s.rope_row0 + s.rows_per_seq <= (long)w.rope, "rope rows read (%s)", what);
            } else {
                EXPECT(s.hn_q_cols == 0 && s.hn_qk_cols == 0 && s.rope_row0 == 0, "head fields outside mode 4 (%s)", what);
            }
            flops += s.flops;
            reads(s, s.src, (long)s.M * s.lda, i);
            writes(s, s.dst, (long)s.M * s.ldc, i);
            break;
        case ACE355_ENC_STEP_KV_STORE:
            EXPECT(cached && s.dst == ACE355_ENC_BUF_CACHE && s.pos0 == r.pos0 && s.pos0 >= 0 && (long)s.pos0 + s.Sq <= r.max_pos && s.seqs <= r.max_seqs, "kv store (%s)", what);
            reads(s, s.src, (long)s.seqs * s.Sq * s.ld, i);
            stored_layer = s.layer;
            break;
        case ACE355_ENC_STEP_DECODE_ATTN: {
            const LmDecodePlan d = plan_lm_decode(r.pos0 + 1);
            EXPECT(decode && S == 1 && s.len == r.pos0 + 1 && s.len <= r.max_pos && s.seqs <= r.max_seqs && s.first == 1 && r.has_first, "decode attention (%s)", what);
            EXPECT(s.chunk == d.chunk && s.splits == d.splits && s.splits >= 1 && s.splits <= LM_MAX_SPLITS && s.chunk % LM_DECODE_KEY_GROUPS == 0 &&
                       (long)s.splits * s.chunk >= s.len && (long)(s.splits - 1) * s.chunk < s.len, "decode cut %d x %d of %d keys (%s)", s.splits, s.chunk, s.len, what);
            EXPECT(stored_layer == s.layer, "decode attention of layer %d before this step's K / V are stored (%s)", s.layer, what);
            EXPECT(r.num_heads == 2 * r.num_kv_heads, "decode attention writes 2 Hkv heads (%s)", what);
            reads(s, s.src, (long)s.seqs * s.ld, i);
            writes(s, s.dst, (long)s.seqs * 2 * s.Hkv * 128, i);
            break;
        }
        case ACE355_ENC_STEP_CAUSAL_ATTN:
            EXPECT(r.causal && !decode && s.first == (cached && r.has_first), "causal attention (%s)", what);
            reads(s, s.src, (long)s.seqs * s.Sq * s.ld, i);
            writes(s, s.dst, (long)s.seqs * s.Sq * s.o_ld, i);
            break;
        case ACE355_ENC_STEP_TRANSPOSE_V:
            EXPECT(!r.causal && s.Sp == f.Sp && s.dst == ACE355_ENC_BUF_VT, "transpose_v (%s)", what);
            reads(s, s.src, (long)s.seqs * s.Sq * s.ld, i);
            writes(s, s.dst, (long)s.seqs * s.Hkv * 128 * s.Sp, i);
            break;
        case ACE355_ENC_STEP_VMEAN:
            EXPECT(!r.causal && r.has_kv_len && s.dst == ACE355_ENC_BUF_VMEAN && w.kvlen >= (size_t)s.seqs, "vmean (%s)", what);
            reads(s, s.src, (long)s.seqs * s.Sq * s.ld, i);
            writes(s, s.dst, (long)s.seqs * s.Hkv * 128, i);
            break;
        case ACE355_ENC_STEP_ATTN:
            EXPECT(!r.causal && s.Skv == S && s.Sp == f.Sp && s.kv_len == (r.has_kv_len != 0), "attention (%s)", what);
            // 5. the layer's window
            EXPECT(s.window == (((r.sliding_layer_mask >> s.layer) & 1ull) ? r.sliding_window : -1), "window of layer %d (%s)", s.layer, what);
            // (the last key tile of the last sequence is read in whole 64-row tiles with clamped rows: up to Sp rows from its first)
            reads(s, s.src, ((long)(s.seqs - 1) * s.Sq + s.Sp) * s.ld, i);
            reads(s, ACE355_ENC_BUF_VT, (long)s.seqs * s.Hkv * 128 * s.Sp, i);
            if (s.kv_len) reads(s, ACE355_ENC_BUF_VMEAN, (long)s.seqs * s.Hkv * 128, i);
            writes(s, s.dst, (long)s.seqs * s.Sq * s.o_ld, i);
            break;
        }
    }
    // 6. closed forms
    const long want[ACE355_ENC_STEP_KINDS] = {2 * NL + 1, 4 * NL, cached ? NL : 0, r.causal && !decode ? NL : 0, decode ? NL : 0, r.causal ? 0 : NL,
                                              !r.causal && r.has_kv_len ? NL : 0, r.causal ? 0 : NL};
    for (int k = 0; k < ACE355_ENC_STEP_KINDS; ++k) EXPECT(calls[k] == want[k] && f.calls[k] == want[k], "calls of kind %d: %d, closed form %ld (%s)", k, calls[k], want[k], what);
    const double want_flops = NL * (2.0 * M * QKV * D + 2.0 * M * D * QD + 2.0 * M * 2 * F * D + 2.0 * M * D * F);
    EXPECT(flops == want_flops && f.gemm_flops == want_flops, "GEMM FLOPs %.0f, closed form %.0f (%s)", flops, want_flops, what);
    // 7. again: equal, and into the same plan without a reallocation
    const EncPassPlan q = plan_encoder_pass(r);
    EXPECT(!q.error && q.steps.size() == p.steps.size() && memcmp(&q.info, &p.info, sizeof p.info) == 0 &&
               (p.steps.empty() || memcmp(q.steps.data(), p.steps.data(), p.steps.size() * sizeof(EncStep)) == 0), "two calls, two plans (%s)", what);
    const EncStep* data = p.steps.data();
    const size_t cap = p.steps.capacity();
    plan_encoder_pass(r, p);
    EXPECT(p.steps.data() == data && p.steps.capacity() == cap && p.steps.size() == q.steps.size(), "replanning reallocated the steps (%s)", what);
}

static void expect_refusal(EncPassRequest r, const char* text) {
    const EncPassPlan p = plan_encoder_pass(r);
    ++g_refused;
    EXPECT(p.error && strcmp(p.error, text) == 0 && p.steps.empty(), "wanted the refusal '%s', got '%s'", text, p.error ? p.error : "(a plan)");
}

int main() {
    struct Dims { int D, F, HQ, KVH, NL; };
    const Dims dims[] = {{256, 768, 2, 1, 2}, {256, 768, 2, 1, 0}, {256, 512, 4, 2, 3}, {1024, 3072, 16, 8, 28}, {2048, 6144, 16, 8, 4}, {512, 1536, 6, 2, 5},
                         {256, 768, 2, 1, 70}};
    const int Ns[] = {1, 2, 3, 16, 65}, Ss[] = {1, 63, 64, 65, 130};
    char what[256];
    for (const Dims& d : dims) {
        EncPassRequest base{};
        base.hidden_size = d.D; base.intermediate_size = d.F; base.num_heads = d.HQ; base.num_kv_heads = d.KVH; base.num_layers = d.NL;
        for (int N : Ns) {
            // ---- bidirectional: with and without key counts, no window / some layers sliding / all
            if (d.NL <= 64)
                for (int S : Ss)
                    for (int kv = 0; kv < 2; ++kv)
                        for (unsigned long long mask : {0ull, 0x5ull, ~0ull}) {
                            EncPassRequest r = base;
                            r.N = N; r.S = S; r.has_kv_len = kv; r.sliding_window = 128; r.sliding_layer_mask = mask;
                            snprintf(what, sizeof what, "bidirectional D %d NL %d N %d S %d kv %d mask %llx", d.D, d.NL, N, S, kv, mask);
                            check_pass(r, what);
                        }
            if (d.HQ != 2 * d.KVH) continue;   // the causal kernels' head layout (textenc_create, lm_create)
            // ---- causal over the QKV rows; the mask is not read (70 layers: more than it has bits)
            for (int S : Ss) {
                EncPassRequest r = base;
                r.causal = 1; r.N = N; r.S = S; r.sliding_layer_mask = ~0ull; r.sliding_window = 7;
                snprintf(what, sizeof what, "causal D %d NL %d N %d S %d", d.D, d.NL, N, S);
                check_pass(r, what);
            }
            // ---- with a cache: prefills (pos0 == 0) up to pos0 + S == max_pos, decode steps across the regime boundaries and at the last position
            if (N > 16) continue;
            for (int max_seqs : {N, 16})
                for (int first = 0; first < 2; ++first) {
                    for (int S : Ss)
                        for (int max_pos : {S, S + 7, 2048}) {
                            EncPassRequest r = base;
                            r.causal = 1; r.N = N; r.S = S; r.has_cache = 1; r.pos0 = 0; r.max_pos = max_pos; r.max_seqs = max_seqs; r.has_first = first;
                            snprintf(what, sizeof what, "prefill D %d NL %d N %d S %d max_pos %d first %d", d.D, d.NL, N, S, max_pos, first);
                            check_pass(r, what);
                        }
                    for (int len : {2, 64, 65, 255, 256, 257, 258, 1023, 1024, 1025, 1026, 4096, 16384})
                        for (int max_pos : {len, len + 1, 16384}) {
                            EncPassRequest r = base;
                            r.causal = 1; r.N = N; r.S = 1; r.has_cache = 1; r.pos0 = len - 1; r.max_pos = max_pos; r.max_seqs = max_seqs; r.has_first = first;
                            snprintf(what, sizeof what, "decode D %d NL %d N %d len %d max_pos %d first %d", d.D, d.NL, N, len, max_pos, first);
                            if (first || d.NL == 0) check_pass(r, what);
                            else expect_refusal(r, "decode attention: cache bounds");
                        }
                }
        }
    }
    // ---- a call's workspace covers each of its passes (the condition encoder's two)
    {
        EncPassRequest a{}, b{};
        a.hidden_size = b.hidden_size = 256; a.intermediate_size = b.intermediate_size = 768; a.num_heads = b.num_heads = 2; a.num_kv_heads = b.num_kv_heads = 1;
        a.num_layers = 2; b.num_layers = 1; a.N = 3; a.S = 70; a.has_kv_len = 1; b.N = 5; b.S = 200;
        const EncPassRequest both[2] = {a, b};
        const EncWorkspacePlan w = plan_encoder_workspace(both, 2, 1234, 56);
        EXPECT(enc_pass_need(a).within(w.need) && enc_pass_need(b).within(w.need) && w.in_bf == 1234 && w.emb == 56 * 256 && w.need.rows == 1000 &&
                   w.vt == 5 * 128 * 256 && w.vmean == 3 * 128 && w.kvlen == 3 && w.need.rope_rows == 200 && w.rope == 512, "the workspace of two passes");
        EXPECT(!w.need.within(enc_pass_need(a)) && w.need.within(w.need.max_with(enc_pass_need(a))), "grow-only");
    }
    // ---- refusals, with the texts the stack and its launchers give
    {
        EncPassRequest r{};
        r.hidden_size = 256; r.intermediate_size = 768; r.num_heads = 2; r.num_kv_heads = 1; r.num_layers = 2; r.N = 2; r.S = 1;
        r.causal = 1; r.has_cache = 1; r.max_pos = 32; r.max_seqs = 2; r.has_first = 1;
        EncPassRequest q = r;
        q.pos0 = 32; expect_refusal(q, "encoder_layers: KV cache position");              // past the end
        q = r; q.pos0 = -1; expect_refusal(q, "encoder_layers: KV cache position");
        q = r; q.pos0 = 3; q.S = 2; expect_refusal(q, "encoder_layers: KV cache position");   // a decode step is one row
        q = r; q.S = 33; expect_refusal(q, "encoder_layers: KV cache position");
        q = r; q.causal = 0; expect_refusal(q, "encoder_layers: KV cache position");       // a cache on a bidirectional stack
        q = r; q.N = 3; expect_refusal(q, "kv store: cache bounds");
        q = r; q.has_cache = 0; q.N = 65536; expect_refusal(q, "causal attention: sizes");
        q = r; q.hidden_size = 288; expect_refusal(q, "gemm: K must be a multiple of 64");
        q = r; q.has_cache = 0; q.N = 1 << 12; q.S = 1 << 12; expect_refusal(q, "gemm: A and W must each be smaller than 4 GB (32-bit DMA offsets)");
        q = r; q.has_cache = 0; q.causal = 0; q.num_heads = 3; q.num_kv_heads = 2; expect_refusal(q, "attention: Hq % Hkv");
        q = r; q.has_cache = 0; q.N = 0; expect_refusal(q, "encoder_layers: sizes");
    }
    printf("pass plans: %ld planned (%ld steps), %ld refused; failures: %ld\n", g_plans, g_steps, g_refused, g_fail);
    return g_fail ? 1 : 0;
}
