// encoder_plan.h - the host side of the encoder stack (encoder.hip) as data, in the shape of dit_plan.h: the launcher calls of one pass in
// order (EncPassRequest -> EncPassPlan, plan_encoder_pass) with everything a call takes except pointers, and the element counts of the
// workspace and the rope tables for a set of passes (plan_encoder_workspace).  encoder.hip executes the first (run_encoder_pass) and
// allocates from the second (ensure_workspace).  Pure functions: no HIP call, no global, no environment - ace355_encoder_pass_plan
// answers on a machine without a GPU, and the header compiles with a plain host compiler.
//
// Three attention paths, chosen by the request alone:
//   bidirectional (cond, detok, tok): transpose_v, vmean when key counts are given, launch_attention with the layer's window
//   causal over the QKV rows (textenc; the LM's prefill, which also stores K / V and binds the first visible keys)
//   causal over the cache (an LM decode step, pos0 > 0 and S == 1): store, then pos0 + 1 keys cut by plan_lm_decode
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/ace355.h"
#include "lm_plan.h"

namespace ace355 {

using EncPassRequest = ace355_encoder_pass_request;
using EncStep = ace355_encoder_step_info;

struct EncPassPlan {
    const char* error = nullptr;       // the refusal, with the text the stack or the launcher gave; nothing else is set then
    ace355_encoder_pass_info info{};   // M, Sp, QKV, rope_rows, the counts
    std::vector<EncStep> steps;        // in launch order
};

constexpr int ENC_QKV_PAD_ROWS = 64;   // rows of qkv behind the M of the call: the last K tile's DMA rows are clamped, not skipped (gemm.hip)

inline long enc_round64(long v) { return ((v + 63) / 64) * 64; }

// Planned into `p`, whose step vector keeps its capacity: an LM decode step replans on every token without an allocation.
inline void plan_encoder_pass(const EncPassRequest& r, EncPassPlan& p) {
    p.error = nullptr;
    p.info = ace355_encoder_pass_info{};
    p.steps.clear();
    const long N = r.N, S = r.S, M = N * S, Sp = enc_round64(S);
    const long D = r.hidden_size, F = r.intermediate_size, HQ = r.num_heads, KVH = r.num_kv_heads, NL = r.num_layers;
    const long QD = HQ * 128, KVD = KVH * 128, QKV = QD + 2 * KVD;
    const bool cached = r.has_cache != 0, decode = cached && r.pos0 > 0;
    auto refuse = [&](const char* text) { p.error = text; };
    // ---- the rules of encoder_layers and of the launchers it calls, in the order a pass would meet them
    if (cached && !(r.causal && r.pos0 >= 0 && (long)r.pos0 + S <= r.max_pos && (r.pos0 == 0 || S == 1))) return refuse("encoder_layers: KV cache position");
    // (no caller reaches the next one: every entry point checks its sizes first.  It keeps the arithmetic below inside an int.)
    if (N <= 0 || S <= 0 || D <= 0 || F <= 0 || HQ <= 0 || KVH <= 0 || NL < 0 || M >= (1L << 31)) return refuse("encoder_layers: sizes");
    if (D % 4 != 0) return refuse("rmsnorm: D % 4");
    if (NL > 0) {
        const long a_max = D > QD ? (D > F ? D : F) : (QD > F ? QD : F);   // the widest A operand: xn, ao, act
        if (D % 64 != 0 || F % 64 != 0) return refuse("gemm: K must be a multiple of 64");
        if (M * a_max >= (1L << 31) || QKV * D >= (1L << 31) || 2 * F * D >= (1L << 31))
            return refuse("gemm: A and W must each be smaller than 4 GB (32-bit DMA offsets)");
        if (r.causal) {
            if (cached && N > r.max_seqs) return refuse("kv store: cache bounds");
            if (decode && !r.has_first) return refuse("decode attention: cache bounds");
            if (decode && plan_lm_decode(r.pos0 + 1).splits > LM_MAX_SPLITS) return refuse("decode attention: plan");
            if (!decode && (N > 65535 || KVH > 65535)) return refuse("causal attention: sizes");
            // the two causal kernels share a K / V read among 2 or 4 q heads (textenc.hip, lm.hip); no other layout is built
            if (HQ != 2 * KVH && HQ != 4 * KVH) return refuse("causal attention: 2 or 4 q heads per kv head");
        } else {
            if (HQ % KVH != 0) return refuse("attention: Hq % Hkv");
        }
    }
    ace355_encoder_pass_info& f = p.info;
    f.M = (int)M; f.Sp = (int)Sp; f.QKV = (int)QKV;
    f.rope_rows = cached ? r.max_pos : (int)S;   // row s of the call is position pos0 + s <= max_pos - 1

    auto blank = [](int kind, int layer, int src, int dst) {
        EncStep s{};
        s.kind = kind; s.layer = layer; s.src = src; s.dst = dst;
        s.norm = -1; s.proj = -1; s.window = -1;
        return s;
    };
    auto push = [&](const EncStep& s) {
        f.calls[s.kind]++;
        p.steps.push_back(s);
    };
    auto norm = [&](int layer, int which, int dst) {
        EncStep s = blank(ACE355_ENC_STEP_RMSNORM, layer, ACE355_ENC_BUF_H, dst);
        s.norm = which; s.M = (int)M; s.N = (int)D; s.rows_per_seq = (int)S;
        push(s);
    };
    auto gemm = [&](int layer, int proj, int src, int dst, long n, long k, long ldc, int mode, long rows_per_seq) {
        EncStep s = blank(ACE355_ENC_STEP_GEMM, layer, src, dst);
        s.proj = proj; s.M = (int)M; s.N = (int)n; s.K = (int)k; s.lda = s.ldw = (int)k; s.ldc = (int)ldc; s.mode = mode;
        s.rows_per_seq = (int)rows_per_seq;
        if (mode == 4) { s.hn_q_cols = (int)QD; s.hn_qk_cols = (int)(QD + KVD); s.rope_row0 = cached ? r.pos0 : 0; }
        s.sk_cnt = mode == 2;
        s.flops = 2.0 * M * n * (double)k;
        f.gemm_flops += s.flops;
        push(s);
    };
    // kv_store, the attentions, transpose_v and vmean all read the QKV rows
    auto rows = [&](int kind, int layer, int dst) {
        EncStep s = blank(kind, layer, ACE355_ENC_BUF_QKV, dst);
        s.seqs = (int)N; s.Sq = s.Skv = (int)S; s.Hq = (int)HQ; s.Hkv = (int)KVH;
        s.ld = (int)QKV; s.k_col0 = (int)QD; s.v_col0 = (int)(QD + KVD); s.o_ld = (int)QD;
        return s;
    };
    const int XN = ACE355_ENC_BUF_XN, AO = ACE355_ENC_BUF_AO, H = ACE355_ENC_BUF_H;
    for (int li = 0; li < NL; ++li) {
        // ---- self attention (base.py:414-427): q / k head-norm + RoPE in the QKV epilogue, as in the DiT
        norm(li, 0, XN);
        gemm(li, ACE355_ENC_PROJ_QKV, XN, ACE355_ENC_BUF_QKV, QKV, D, QKV, 4, S);
        if (r.causal) {   // (a causal stack may have more layers than sliding_layer_mask has bits: the mask is not read here)
            if (cached) {
                EncStep s = rows(ACE355_ENC_STEP_KV_STORE, li, ACE355_ENC_BUF_CACHE);
                s.pos0 = r.pos0;
                push(s);
            }
            if (decode) {
                EncStep s = rows(ACE355_ENC_STEP_DECODE_ATTN, li, AO);
                const LmDecodePlan d = plan_lm_decode(r.pos0 + 1);
                s.len = s.Skv = r.pos0 + 1; s.chunk = d.chunk; s.splits = d.splits; s.first = 1;
                push(s);
            } else {
                EncStep s = rows(ACE355_ENC_STEP_CAUSAL_ATTN, li, AO);
                s.first = cached && r.has_first;
                push(s);
            }
        } else {
            EncStep t = rows(ACE355_ENC_STEP_TRANSPOSE_V, li, ACE355_ENC_BUF_VT);
            t.Sp = (int)Sp;
            push(t);
            if (r.has_kv_len) push(rows(ACE355_ENC_STEP_VMEAN, li, ACE355_ENC_BUF_VMEAN));
            EncStep a = rows(ACE355_ENC_STEP_ATTN, li, AO);
            a.Sp = (int)Sp; a.kv_len = r.has_kv_len != 0;
            a.window = li < 64 && ((r.sliding_layer_mask >> li) & 1ull) ? r.sliding_window : -1;
            push(a);
        }
        gemm(li, ACE355_ENC_PROJ_O, AO, H, D, QD, D, 2, S);   // h += o_proj(attn)
        // ---- SwiGLU MLP (base.py:430-433)
        norm(li, 1, XN);
        gemm(li, ACE355_ENC_PROJ_GATE_UP, XN, ACE355_ENC_BUF_ACT, 2 * F, D, F, 3, 0);
        gemm(li, ACE355_ENC_PROJ_DOWN, ACE355_ENC_BUF_ACT, H, D, F, D, 2, S);
    }
    norm(-1, 2, ACE355_ENC_BUF_OUT);
    f.n_steps = (int)p.steps.size();
}

inline EncPassPlan plan_encoder_pass(const EncPassRequest& r) {
    EncPassPlan p;
    plan_encoder_pass(r, p);
    return p;
}

// ------------------------------------------------------------------------------------------------ buffer sizes
// What a handle's workspace is measured in: the largest of each over the calls so far (grow-only, encoder.hip ensure_workspace).
struct EncWorkspaceNeed {
    long rows = 0;       // M of the largest pass: h, xn, qkv (+ ENC_QKV_PAD_ROWS), ao, act
    long in_elems = 0;   // the caller's input as bf16 (in_bf)
    long emb_rows = 0;   // the caller's embedded rows ahead of the stack (emb, x D)
    long vt_elems = 0;   // bidirectional passes: N * KVH * 128 * Sp
    long seqs = 0;       // passes with key counts: N (vmean x KVD, kvlen)
    long rope_rows = 0;  // rows of the rope tables
    bool within(const EncWorkspaceNeed& held) const {
        return rows <= held.rows && in_elems <= held.in_elems && emb_rows <= held.emb_rows && vt_elems <= held.vt_elems && seqs <= held.seqs &&
               rope_rows <= held.rope_rows;
    }
    EncWorkspaceNeed max_with(const EncWorkspaceNeed& o) const {
        auto mx = [](long a, long b) { return a > b ? a : b; };
        EncWorkspaceNeed n;
        n.rows = mx(rows, o.rows); n.in_elems = mx(in_elems, o.in_elems); n.emb_rows = mx(emb_rows, o.emb_rows);
        n.vt_elems = mx(vt_elems, o.vt_elems); n.seqs = mx(seqs, o.seqs); n.rope_rows = mx(rope_rows, o.rope_rows);
        return n;
    }
};
// One pass's share.  (A refused request needs nothing: the pass will not run.)
inline EncWorkspaceNeed enc_pass_need(const EncPassRequest& r) {
    EncWorkspaceNeed n;
    const bool cached = r.has_cache != 0;
    if (r.N <= 0 || r.S <= 0) return n;
    n.rows = (long)r.N * r.S;
    if (!r.causal) n.vt_elems = (long)r.N * r.num_kv_heads * 128 * enc_round64(r.S);
    if (!r.causal && r.has_kv_len) n.seqs = r.N;
    n.rope_rows = cached ? r.max_pos : r.S;
    return n;
}
// Element counts of the buffers for a need (ensure_workspace allocates exactly these; 0: the buffer is not allocated)
struct EncWorkspacePlan {
    EncWorkspaceNeed need;
    size_t h, xn, qkv, ao, act, in_bf, emb, vt, vmean, kvlen;
    size_t rope;   // rows the rope tables are allocated for (x 64 floats each): the capacity doubles from 512
};
inline long enc_rope_capacity(long rows) {
    long cap = 512;
    while (cap < rows) cap *= 2;
    return cap;
}
inline EncWorkspacePlan enc_workspace_sizes(int hidden, int intermediate, int heads, int kv_heads, const EncWorkspaceNeed& n) {
    const size_t D = hidden, F = intermediate, QD = (size_t)heads * 128, KVD = (size_t)kv_heads * 128;
    const size_t R = (size_t)n.rows;
    EncWorkspacePlan w{};
    w.need = n;
    w.h = R * D; w.xn = R * D; w.qkv = (R + ENC_QKV_PAD_ROWS) * (QD + 2 * KVD); w.ao = R * QD; w.act = R * F;
    w.in_bf = (size_t)n.in_elems; w.emb = (size_t)n.emb_rows * D; w.vt = (size_t)n.vt_elems;
    w.vmean = (size_t)n.seqs * KVD; w.kvlen = (size_t)n.seqs;
    w.rope = n.rope_rows > 0 ? (size_t)enc_rope_capacity(n.rope_rows) : 0;
    return w;
}
// ... for the passes of one call (all on one handle: the dimensions are the first request's) plus the caller's own two buffers
inline EncWorkspacePlan plan_encoder_workspace(const EncPassRequest* passes, int n_passes, long in_elems, long emb_rows) {
    EncWorkspaceNeed n;
    n.in_elems = in_elems;
    n.emb_rows = emb_rows;
    for (int i = 0; i < n_passes; ++i) n = n.max_with(enc_pass_need(passes[i]));
    return enc_workspace_sizes(passes[0].hidden_size, passes[0].intermediate_size, passes[0].num_heads, passes[0].num_kv_heads, n);
}

}  // namespace ace355
