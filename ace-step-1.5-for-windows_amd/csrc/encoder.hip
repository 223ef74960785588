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

static int ensure_rope(EncBase* h, int S, hipStream_t s) {
    if (S <= h->rope_S) return 0;
    int cap = 512;
    while (cap < S) cap *= 2;
    ALLOC(h->allocs, h->rope_cos, (size_t)cap * 64);
    ALLOC(h->allocs, h->rope_sin, (size_t)cap * 64);
    int rc = launch_rope_table(h->rope_cos, h->rope_sin, cap, h->theta, s);
    if (rc) return rc;
    h->rope_S = cap;
    if (!h->sk_cnt) {
        ALLOC(h->allocs, h->sk_cnt, SK_CNT_INTS);
        ACE_HIP(hipMemsetAsync(h->sk_cnt, 0, SK_CNT_INTS * sizeof(int), s));
        if (int prc = gemm_verify_splitk_placement()) return prc;
    }
    return 0;
}

int ensure_workspace(EncBase* h, long rows, long in_elems, long emb_rows, int seqs, long vt_elems, hipStream_t s) {
    if (rows <= h->ws_rows && in_elems <= h->ws_in && emb_rows <= h->ws_emb && seqs <= h->ws_seqs && vt_elems <= h->ws_vt) return 0;
    ACE_HIP(hipStreamSynchronize(s));
    for (void* p : h->ws_allocs) hipFree(p);
    h->ws_allocs.clear();
    const long R = std::max(rows, h->ws_rows), I = std::max(in_elems, h->ws_in), E = std::max(emb_rows, h->ws_emb),
               V = std::max(vt_elems, h->ws_vt);
    const int Q = std::max(seqs, h->ws_seqs);
    const long D = h->D, QKV = h->QD + 2 * h->KVD;
    h->ws_rows = h->ws_in = h->ws_emb = h->ws_vt = 0;
    h->ws_seqs = 0;
    ALLOC(h->ws_allocs, h->h, (size_t)R * D);
    ALLOC(h->ws_allocs, h->xn, (size_t)R * D);
    ALLOC(h->ws_allocs, h->qkv, (size_t)(R + 64) * QKV);  // +64 rows: the last K tile's DMA rows are clamped, not skipped
    ALLOC(h->ws_allocs, h->ao, (size_t)R * h->QD);
    ALLOC(h->ws_allocs, h->act, (size_t)R * h->F);
    if (I) ALLOC(h->ws_allocs, h->in_bf, (size_t)I);
    if (E) ALLOC(h->ws_allocs, h->emb, (size_t)E * D);
    if (V) ALLOC(h->ws_allocs, h->vt, (size_t)V);
    if (Q) {
        ALLOC(h->ws_allocs, h->vmean, (size_t)Q * h->KVD);
        ALLOC(h->ws_allocs, h->kvlen_dev, (size_t)Q);
    }
    h->ws_rows = R;
    h->ws_in = I;
    h->ws_emb = E;
    h->ws_seqs = Q;
    h->ws_vt = V;
    return 0;
}

int encoder_layers(EncBase* h, const EncoderW& E, int N, int S, const int* kv_len_dev, bf16_t* out, hipStream_t s, const KvCache* cache) {
    const int M = N * S, D = h->D, F = h->F, QD = h->QD, KVD = h->KVD, QKV = QD + 2 * KVD;
    const int Sp = ((S + 63) / 64) * 64;
    const float eps = h->eps;
    const float scale = 1.0f / sqrtf(128.0f);
    ACE_CHECK(!cache || (h->causal && cache->pos0 >= 0 && cache->pos0 + S <= cache->max_pos && (cache->pos0 == 0 || S == 1)),
              "encoder_layers: KV cache position");
    int rc = ensure_rope(h, cache ? cache->max_pos : S, s);
    if (rc) return rc;
    const long rope0 = cache ? (long)cache->pos0 * 64 : 0;   // row s of the call is position pos0 + s
    GemmEpilogue ep{};
    for (int li = 0; li < E.n_layers; ++li) {
        const EncLayerW& W = E.layers[li];
        // self attention (base.py:414-427)
        rc = launch_rmsnorm_mod(h->h, W.n_in, h->xn, M, D, eps, nullptr, nullptr, nullptr, nullptr, 0, S, s);
        if (rc) return rc;
        ep = GemmEpilogue{4, nullptr, nullptr, nullptr, 0, S};  // q / k head-norm + RoPE in the epilogue, as in the DiT
        ep.hn_wq = W.qn, ep.hn_wk = W.kn, ep.hn_cos = h->rope_cos + rope0, ep.hn_sin = h->rope_sin + rope0;
        ep.hn_q_cols = QD, ep.hn_qk_cols = QD + KVD, ep.hn_eps = eps;
        rc = launch_gemm(h->xn, D, W.wqkv, D, h->qkv, QKV, M, QKV, D, ep, s);
        if (rc) return rc;
        if (h->causal) {   // (a causal stack may have more layers than sliding_layer_mask has bits: the mask is not read here)
            if (cache) {
                rc = launch_kv_store(h->qkv, QKV, QD, QD + KVD, *cache, li, N, S, h->KVH, s);
                if (rc) return rc;
            }
            if (cache && cache->pos0 > 0)
                rc = launch_decode_attention(h->qkv, QKV, *cache, li, cache->pos0 + 1, h->ao, N, h->KVH, scale, s);
            else
                rc = launch_causal_attention(h->qkv, QKV, QD, QD + KVD, h->ao, QD, N, S, h->KVH, scale, s, cache ? cache->first_dev : nullptr);
            if (rc) return rc;
        } else {
            const bool sliding = (h->sliding_layer_mask >> li) & 1ull;
            rc = launch_transpose_v(h->qkv, QKV, QD + KVD, N, S, h->KVH, h->vt, Sp, s);
            if (rc) return rc;
            if (kv_len_dev) {
                rc = launch_vmean(h->qkv, QKV, QD + KVD, N, S, h->KVH, h->vmean, s);
                if (rc) return rc;
            }
            AttnArgs a = attn_args_rows(h->qkv, QKV, h->qkv + QD, QKV, h->vt, Sp, h->ao, N, S, S, h->HQ, h->KVH,
                                        sliding ? h->sliding_window : -1, scale);
            a.kv_len = kv_len_dev;
            a.vmean = kv_len_dev ? h->vmean : nullptr;
            rc = launch_attention(a, s);
            if (rc) return rc;
        }
        ep = GemmEpilogue{2, nullptr, nullptr, nullptr, 0, S};  // h += o_proj(attn)
        ep.sk_cnt = h->sk_cnt;
        rc = launch_gemm(h->ao, QD, W.wo, QD, h->h, D, M, D, QD, ep, s);
        if (rc) return rc;
        // SwiGLU MLP (base.py:430-433)
        rc = launch_rmsnorm_mod(h->h, W.n_post, h->xn, M, D, eps, nullptr, nullptr, nullptr, nullptr, 0, S, s);
        if (rc) return rc;
        ep = GemmEpilogue{3, nullptr, nullptr, nullptr, 0, 0};
        rc = launch_gemm(h->xn, D, W.wgu, D, h->act, F, M, 2 * F, D, ep, s);
        if (rc) return rc;
        ep = GemmEpilogue{2, nullptr, nullptr, nullptr, 0, S};
        ep.sk_cnt = h->sk_cnt;
        rc = launch_gemm(h->act, F, W.wdown, F, h->h, D, M, D, F, ep, s);
        if (rc) return rc;
    }
    return launch_rmsnorm_mod(h->h, E.norm, out, M, D, eps, nullptr, nullptr, nullptr, nullptr, 0, S, s);
}

void free_encoder(EncBase* h) {
    free_base(h);
    for (void* p : h->ws_allocs) hipFree(p);
}

}  // namespace ace355
