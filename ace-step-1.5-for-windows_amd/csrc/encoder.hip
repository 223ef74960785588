// encoder.hip - tensor ingestion shared by every weight-owning handle, and the one encoder stack (encoder.h).  Host-side orchestration
// only: every contraction / norm / attention runs on the DiT's kernels (gemm.hip, attn.hip, elementwise.hip) or on textenc.hip's causal one.
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "encoder.h"

namespace ace355 {

// ------------------------------------------------------------------------------------------------ tensor ingestion
bool parse_layer_index(const std::string& name, size_t prefix_len, int n_layers, int* li, std::string* rest) {
    if (name.compare(prefix_len, 7, "layers.") != 0) return false;
    const size_t i0 = prefix_len + 7, dot = name.find('.', i0);
    if (dot == std::string::npos || dot == i0 || dot - i0 > 9) return false;
    const std::string digits = name.substr(i0, dot - i0);
    if (digits.find_first_not_of("0123456789") != std::string::npos) return false;
    const int v = atoi(digits.c_str());
    if (std::to_string(v) != digits || v >= n_layers) return false;
    *li = v;
    *rest = name.substr(dot + 1);
    return true;
}

int unknown_tensor(const char* who, const char* name) {
    set_error(std::string(who) + ": unknown tensor name '" + name + "'");
    return ACE355_ERR_INVALID;
}

int load_packed(LoadBase* h, const PackDest& d, const char* name, const void* data, int dtype, int64_t numel, int is_device, const char* who) {
    if (numel != d.rows * d.cols) {
        set_error(std::string(who) + ": wrong element count for '" + name + "': got " + std::to_string(numel) + ", expected " +
                  std::to_string(d.rows * d.cols));
        return ACE355_ERR_INVALID;
    }
    if (d.ignore) return ACE355_OK;
    const size_t esz = dtype == ACE355_DTYPE_F32 ? 4 : 2;
    const void* src = data;
    if (!is_device) {
        const size_t bytes = (size_t)numel * esz;
        if (bytes > h->stage_bytes) {
            if (h->stage) ACE_HIP(hipFree(h->stage));
            h->stage = nullptr;
            h->stage_bytes = 0;
            ACE_HIP(hipMalloc(&h->stage, bytes));
            h->stage_bytes = bytes;
        }
        ACE_HIP(hipMemcpy(h->stage, data, bytes, hipMemcpyHostToDevice));
        src = h->stage;
    }
    int rc = launch_pack(src, dtype, d.dst, d.is_bf16, d.mode, d.rows, d.cols, d.dst_ld, d.dst_row0, d.p0, d.p1, nullptr);
    if (rc) return rc;
    ACE_HIP(hipDeviceSynchronize());
    h->loaded.insert(name);
    h->finalized = false;
    return ACE355_OK;
}

int finalize_loaded(LoadBase* h, const char* who) {
    if (h->loaded.size() != h->expected_tensors) {
        set_error(std::string(who) + ": " + std::to_string(h->loaded.size()) + " of " + std::to_string(h->expected_tensors) + " tensors loaded");
        return ACE355_ERR_STATE;
    }
    if (h->stage) { hipFree(h->stage); h->stage = nullptr; h->stage_bytes = 0; }
    h->finalized = true;
    return ACE355_OK;
}

void free_base(LoadBase* h) {
    for (void* p : h->allocs) hipFree(p);
    if (h->stage) hipFree(h->stage);
}

// ------------------------------------------------------------------------------------------------ the encoder stack
void enc_init(EncBase* h, int hidden, int intermediate, int heads, int kv_heads, int sliding_window, unsigned long long sliding_layer_mask,
              float eps, float theta) {
    h->D = hidden; h->F = intermediate; h->HQ = heads; h->KVH = kv_heads;
    h->QD = heads * 128; h->KVD = kv_heads * 128;
    h->sliding_window = sliding_window; h->sliding_layer_mask = sliding_layer_mask;
    h->eps = eps; h->theta = theta;
}

int alloc_encoder(EncBase* h, EncoderW& E, int n_layers, int in_dim) {
    const size_t D = h->D, F = h->F, QD = h->QD, KVD = h->KVD;
    E.n_layers = n_layers;
    E.in_dim = in_dim;
    if (in_dim > 0) {
        ALLOC(h->allocs, E.w_embed, D * in_dim);
        ALLOC(h->allocs, E.b_embed, D);
    }
    ALLOC(h->allocs, E.norm, D);
    E.layers.resize(n_layers);
    for (EncLayerW& L : E.layers) {
        ALLOC(h->allocs, L.wqkv, (QD + 2 * KVD) * D);
        ALLOC(h->allocs, L.wo, D * QD);
        ALLOC(h->allocs, L.wgu, 2 * F * D);
        ALLOC(h->allocs, L.wdown, D * F);
        ALLOC(h->allocs, L.n_in, D);
        ALLOC(h->allocs, L.n_post, D);
        ALLOC(h->allocs, L.qn, 128);
        ALLOC(h->allocs, L.kn, 128);
    }
    return 0;
}

bool resolve_encoder_layer(const EncBase& h, EncLayerW& L, const std::string& q, PackDest* d) {
    const long D = h.D, F = h.F, QD = h.QD, KVD = h.KVD;
    auto rows = [&](void* dst, int bf, long r, long c, long ld, long row0) {
        *d = pack_rows(dst, bf, r, c, ld, row0);
        return true;
    };
    if (q == "input_layernorm.weight") return rows(L.n_in, 0, 1, D, D, 0);
    if (q == "post_attention_layernorm.weight") return rows(L.n_post, 0, 1, D, D, 0);
    // q / k rows in head-pair order for the QKV GEMM's head epilogue (common.h PackMode, gemm.hip mode 4)
    if (q == "self_attn.q_proj.weight") { *d = PackDest{L.wqkv, 1, PACK_ROWS_HEADPAIR, QD, D, D, 0, 0, 0}; return true; }
    if (q == "self_attn.k_proj.weight") { *d = PackDest{L.wqkv, 1, PACK_ROWS_HEADPAIR, KVD, D, D, QD, 0, 0}; return true; }
    if (q == "self_attn.v_proj.weight") return rows(L.wqkv, 1, KVD, D, D, QD + KVD);
    if (q == "self_attn.o_proj.weight") return rows(L.wo, 1, D, QD, QD, 0);
    if (q == "self_attn.q_norm.weight") return rows(L.qn, 0, 1, 128, 128, 0);
    if (q == "self_attn.k_norm.weight") return rows(L.kn, 0, 1, 128, 128, 0);
    if (q == "mlp.gate_proj.weight") { *d = PackDest{L.wgu, 1, PACK_ROWS_IL32, F, D, D, 0, 0, 0}; return true; }
    if (q == "mlp.up_proj.weight") { *d = PackDest{L.wgu, 1, PACK_ROWS_IL32, F, D, D, 0, 1, 0}; return true; }
    if (q == "mlp.down_proj.weight") return rows(L.wdown, 1, D, F, F, 0);
    return false;
}

bool resolve_encoder_layers(const EncBase& h, EncoderW& E, const std::string& name, size_t prefix_len, PackDest* d) {
    int li;
    std::string rest;
    return parse_layer_index(name, prefix_len, E.n_layers, &li, &rest) && resolve_encoder_layer(h, E.layers[li], rest, d);
}

EncPassRequest enc_request(const EncBase& h, const EncoderW& E, int N, int S, bool has_kv_len, const KvCache* cache, int pos0) {
    EncPassRequest r{};
    r.hidden_size = h.D; r.intermediate_size = h.F; r.num_heads = h.HQ; r.num_kv_heads = h.KVH; r.num_layers = E.n_layers;
    r.sliding_window = h.sliding_window; r.sliding_layer_mask = h.sliding_layer_mask; r.causal = h.causal;
    r.N = N; r.S = S; r.has_kv_len = has_kv_len;
    if (cache) { r.has_cache = 1; r.pos0 = pos0; r.max_pos = cache->max_pos; r.max_seqs = cache->max_seqs; r.has_first = cache->first_dev != nullptr; }
    return r;
}

static int grow_rope(EncBase* h, size_t cap, hipStream_t s) {
    ALLOC(h->allocs, h->rope_cos, cap * 64);
    ALLOC(h->allocs, h->rope_sin, cap * 64);
    int rc = launch_rope_table(h->rope_cos, h->rope_sin, (int)cap, h->theta, s);
    if (rc) return rc;
    h->ws.rope_rows = (long)cap;
    if (!h->sk_cnt) {
        ALLOC(h->allocs, h->sk_cnt, SK_CNT_INTS);
        ACE_HIP(hipMemsetAsync(h->sk_cnt, 0, SK_CNT_INTS * sizeof(int), s));
        if (int prc = gemm_verify_splitk_placement()) return prc;
    }
    return 0;
}

int ensure_workspace(EncBase* h, const EncWorkspacePlan& want, hipStream_t s) {
    if (want.need.within(h->ws)) return 0;
    if (want.need.rope_rows > h->ws.rope_rows)
        if (int rc = grow_rope(h, want.rope, s)) return rc;
    if (want.need.within(h->ws)) return 0;   // only the tables were short
    ACE_HIP(hipStreamSynchronize(s));
    for (void* p : h->ws_allocs) hipFree(p);
    h->ws_allocs.clear();
    const EncWorkspaceNeed need = want.need.max_with(h->ws);
    h->ws = EncWorkspaceNeed{};
    h->ws.rope_rows = need.rope_rows;
    const EncWorkspacePlan w = enc_workspace_sizes(h->D, h->F, h->HQ, h->KVH, need);
    ALLOC(h->ws_allocs, h->h, w.h);
    ALLOC(h->ws_allocs, h->xn, w.xn);
    ALLOC(h->ws_allocs, h->qkv, w.qkv);
    ALLOC(h->ws_allocs, h->ao, w.ao);
    ALLOC(h->ws_allocs, h->act, w.act);
    if (w.in_bf) ALLOC(h->ws_allocs, h->in_bf, w.in_bf);
    if (w.emb) ALLOC(h->ws_allocs, h->emb, w.emb);
    if (w.vt) ALLOC(h->ws_allocs, h->vt, w.vt);
    if (w.vmean) {
        ALLOC(h->ws_allocs, h->vmean, w.vmean);
        ALLOC(h->ws_allocs, h->kvlen_dev, w.kvlen);
    }
    h->ws = need;
    return 0;
}

// One step = one launcher call; the step names the buffers, the handle and the call have the pointers.
int run_encoder_pass(EncBase* h, const EncoderW& E, const EncPassRequest& rq, const int* kv_len_dev, bf16_t* out, hipStream_t s,
                     const KvCache* cache) {
    EncPassPlan& p = h->plan;
    plan_encoder_pass(rq, p);
    ACE_CHECK(!p.error, p.error);
    ACE_CHECK(rq.num_layers == E.n_layers && !rq.has_kv_len == !kv_len_dev && !rq.has_cache == !cache && out, "encoder pass: the request is not this call's");
    ACE_CHECK(enc_pass_need(rq).within(h->ws), "encoder pass: the workspace does not hold this pass");
    const float eps = h->eps, scale = 1.0f / sqrtf(128.0f);
    auto buf = [&](int b) -> void* {
        switch (b) {
        case ACE355_ENC_BUF_H: return h->h;
        case ACE355_ENC_BUF_XN: return h->xn;
        case ACE355_ENC_BUF_QKV: return h->qkv;
        case ACE355_ENC_BUF_AO: return h->ao;
        case ACE355_ENC_BUF_ACT: return h->act;
        case ACE355_ENC_BUF_VT: return h->vt;
        case ACE355_ENC_BUF_VMEAN: return h->vmean;
        case ACE355_ENC_BUF_OUT: return out;
        default: return nullptr;
        }
    };
    for (const EncStep& st : p.steps) {
        const EncLayerW* W = st.layer >= 0 ? &E.layers[st.layer] : nullptr;
        const bf16_t* qkv = h->qkv;
        int rc = 0;
        switch (st.kind) {
        case ACE355_ENC_STEP_RMSNORM:
            rc = launch_rmsnorm_mod(h->h, st.norm == 0 ? W->n_in : st.norm == 1 ? W->n_post : E.norm, (bf16_t*)buf(st.dst), st.M, st.N, eps, nullptr,
                                    nullptr, nullptr, nullptr, 0, st.rows_per_seq, s);
            break;
        case ACE355_ENC_STEP_GEMM: {
            const bf16_t* w[4] = {W->wqkv, W->wo, W->wgu, W->wdown};
            GemmEpilogue ep{st.mode, nullptr, nullptr, nullptr, 0, st.rows_per_seq};
            if (st.mode == 4) {
                ep.hn_wq = W->qn, ep.hn_wk = W->kn, ep.hn_cos = h->rope_cos + (long)st.rope_row0 * 64, ep.hn_sin = h->rope_sin + (long)st.rope_row0 * 64;
                ep.hn_q_cols = st.hn_q_cols, ep.hn_qk_cols = st.hn_qk_cols, ep.hn_eps = eps;
            }
            if (st.sk_cnt) ep.sk_cnt = h->sk_cnt;
            rc = launch_gemm((const bf16_t*)buf(st.src), st.lda, w[st.proj], st.ldw, buf(st.dst), st.ldc, st.M, st.N, st.K, ep, s);
            break;
        }
        case ACE355_ENC_STEP_KV_STORE: rc = launch_kv_store(qkv, st.ld, st.k_col0, st.v_col0, *cache, st.layer, st.seqs, st.Sq, st.Hkv, st.pos0, s); break;
        case ACE355_ENC_STEP_DECODE_ATTN: rc = launch_decode_attention(qkv, st.ld, *cache, st.layer, st.len, h->ao, st.seqs, st.Hq, st.Hkv, scale, s); break;
        case ACE355_ENC_STEP_CAUSAL_ATTN:
            rc = launch_causal_attention(qkv, st.ld, st.k_col0, st.v_col0, h->ao, st.o_ld, st.seqs, st.Sq, st.Hq, st.Hkv, scale, s, st.first ? cache->first_dev : nullptr);
            break;
        case ACE355_ENC_STEP_TRANSPOSE_V: rc = launch_transpose_v(qkv, st.ld, st.v_col0, st.seqs, st.Sq, st.Hkv, h->vt, st.Sp, s); break;
        case ACE355_ENC_STEP_VMEAN: rc = launch_vmean(qkv, st.ld, st.v_col0, st.seqs, st.Sq, st.Hkv, h->vmean, s); break;
        case ACE355_ENC_STEP_ATTN: {
            AttnArgs a = attn_args_rows(qkv, st.ld, qkv + st.k_col0, st.ld, h->vt, st.Sp, h->ao, st.seqs, st.Sq, st.Skv, st.Hq, st.Hkv, st.window, scale);
            a.kv_len = st.kv_len ? kv_len_dev : nullptr;
            a.vmean = st.kv_len ? h->vmean : nullptr;
            rc = launch_attention(a, s);
            break;
        }
        default: ACE_CHECK(false, "encoder pass: unknown step kind");
        }
        if (rc) return rc;
    }
    return 0;
}

void free_encoder(EncBase* h) {
    free_base(h);
    for (void* p : h->ws_allocs) hipFree(p);
}

}  // namespace ace355
