// encoder.h - what the weight-owning handles share (encoder.hip): tensor ingestion (staging, packing, the loaded-set bookkeeping of
// load_tensor / finalize / destroy) for every handle, and the pre-norm encoder stack behind five handles - ace355_cond (two stacks),
// ace355_detok, ace355_tok, ace355_textenc and ace355_lm: RMSNorm, QKV GEMM with head-norm + RoPE in its epilogue, attention, h += o_proj,
// RMSNorm, SwiGLU gate|up GEMM, h += down.  Which launches a pass makes, and how large the workspace has to be, is encoder_plan.h's.
#pragma once
#include <set>
#include <string>
#include <vector>

#include "../../include/ace355.h"
#include "common.h"
#include "encoder_plan.h"

namespace ace355 {

// ------------------------------------------------------------------------------------------------ device allocations
template <typename T>
int dev_alloc(std::vector<void*>& bag, T** p, size_t n) {
    void* q = nullptr;
    ACE_HIP(hipMalloc(&q, n * sizeof(T) + 256));
    bag.push_back(q);
    *p = reinterpret_cast<T*>(q);
    return 0;
}
#define ALLOC(bag, ptr, n)                     \
    do {                                       \
        int _rc = dev_alloc(bag, &(ptr), (n)); \
        if (_rc) return _rc;                   \
    } while (0)

// ------------------------------------------------------------------------------------------------ tensor ingestion
// base of every handle that is filled through *_load_tensor and sealed by *_finalize
struct LoadBase {
    std::set<std::string> loaded;
    size_t expected_tensors = 0;
    bool finalized = false;
    std::vector<void*> allocs;   // weights (and whatever else lives as long as the handle)
    void* stage = nullptr;       // device staging of a host tensor on its way through launch_pack
    size_t stage_bytes = 0;
};

// packed destination of one state-dict tensor (launch_pack arguments); `ignore`: a key that is accepted and dropped
struct PackDest {
    void* dst;
    int is_bf16, mode;
    long rows, cols, dst_ld, dst_row0;
    int p0, p1;
    bool ignore = false;
};
inline PackDest pack_rows(void* dst, int is_bf16, long rows, long cols, long dst_ld, long dst_row0) {
    return PackDest{dst, is_bf16, PACK_ROWS, rows, cols, dst_ld, dst_row0, 0, 0};
}

// "<prefix>layers.<i>.<rest>" with <i> in canonical decimal form (no sign, no leading zero) and below n_layers; anything else is not a
// layer key.  prefix_len: characters of `name` in front of "layers.".
bool parse_layer_index(const std::string& name, size_t prefix_len, int n_layers, int* li, std::string* rest);
// Element-count check, host -> staging copy, launch_pack, sync, and the loaded-set entry.  Errors read "<who>: ...".
int load_packed(LoadBase* h, const PackDest& d, const char* name, const void* data, int dtype, int64_t numel, int is_device, const char* who);
int unknown_tensor(const char* who, const char* name);       // sets "<who>: unknown tensor name '<name>'"
int finalize_loaded(LoadBase* h, const char* who);           // every expected tensor loaded -> drop the staging buffer, finalized
void free_base(LoadBase* h);                                 // allocs + staging buffer

// ------------------------------------------------------------------------------------------------ the encoder stack
struct EncLayerW {
    bf16_t *wqkv, *wo, *wgu, *wdown;
    float *n_in, *n_post, *qn, *kn;
};
struct EncoderW {
    int n_layers = 0, in_dim = 0;
    bf16_t* w_embed = nullptr;   // input Linear [D][in_dim] (+ b_embed); absent when in_dim == 0
    float *b_embed = nullptr, *norm = nullptr;
    std::vector<EncLayerW> layers;
};

// state shared by every encoder-stack handle: dimensions, workspace, rope tables
struct EncBase : LoadBase {
    int D = 0, F = 0, QD = 0, KVD = 0, HQ = 0, KVH = 0, sliding_window = 0;
    unsigned long long sliding_layer_mask = 0;   // bidirectional stacks only (<= 64 layers)
    float eps = 1e-6f, theta = 1e6f;
    bool causal = false;   // attention of a pass: causal over the QKV rows (textenc.hip) or bidirectional (attn.hip)

    // workspace, sized for the largest call so far (ws: what is held; encoder_plan.h: EncWorkspacePlan).  Every stack: h, xn, qkv, ao, act
    // (by rows).  Bidirectional attention: vt; with key counts vmean, kvlen_dev.  Input Linear: in_bf, emb.
    EncWorkspaceNeed ws;
    std::vector<void*> ws_allocs;
    float *h = nullptr, *emb = nullptr;
    bf16_t *xn = nullptr, *qkv = nullptr, *ao = nullptr, *act = nullptr, *in_bf = nullptr, *vt = nullptr, *vmean = nullptr;
    int* kvlen_dev = nullptr;
    float *rope_cos = nullptr, *rope_sin = nullptr;   // ws.rope_rows rows
    int* sk_cnt = nullptr;   // split-K counters (GemmEpilogue::sk_cnt), allocated with the rope tables
    EncPassPlan plan;        // the pass in progress; kept for the capacity of its step vector
};

void enc_init(EncBase* h, int hidden, int intermediate, int heads, int kv_heads, int sliding_window, unsigned long long sliding_layer_mask,
              float eps, float theta);
// norm + n_layers x the eight layer tensors, and the input Linear when in_dim > 0
int alloc_encoder(EncBase* h, EncoderW& E, int n_layers, int in_dim);
// "<prefix>layers.<i>.<one of the 11 layer keys>" -> its packed destination
bool resolve_encoder_layer(const EncBase& h, EncLayerW& L, const std::string& key_after_index, PackDest* d);
bool resolve_encoder_layers(const EncBase& h, EncoderW& E, const std::string& name, size_t prefix_len, PackDest* d);
// KV cache of a causal stack that is run in steps (lm.hip): bf16 [layer][K | V][max_seqs][kv head][max_pos][128], K as the QKV epilogue
// leaves it (head-normed, rotated, head-pair dim order), V in natural order.  Handed to run_encoder_pass with a request that names pos0,
// rows s of the call sit at positions pos0 + s: their K / V are stored, and a step with pos0 > 0 (S == 1) attends the cache instead of the
// QKV rows.
struct KvCache {
    bf16_t* kv = nullptr;
    int max_seqs = 0, max_pos = 0;
    const int* first_dev = nullptr;   // [N]: first visible key of each sequence (left padding), device
    float *part_o = nullptr, *part_ml = nullptr;   // decode attention's per-chunk partials (lm_plan.h): [N][HQ][LM_MAX_SPLITS][128 | 2]
    long slab(int kvh_count) const { return (long)max_seqs * kvh_count * max_pos * 128; }   // elements of one layer's K (or V)
};

// A pass of `E` on this handle as a request: the handle's dimensions, the call's N x S, and what is bound.  pos0: position of the call's
// first row in `cache` (null: no cache).
EncPassRequest enc_request(const EncBase& h, const EncoderW& E, int N, int S, bool has_kv_len = false, const KvCache* cache = nullptr,
                           int pos0 = 0);
// Grow-only workspace and rope tables: a plan beyond what is held syncs the stream, frees the workspace and reallocates at the max of old
// and new; the rope tables grow on their own (capacity doubling from 512, the old ones stay alive for launches in flight).
int ensure_workspace(EncBase* h, const EncWorkspacePlan& w, hipStream_t s);
// plan_encoder_pass(rq), executed: n_layers x encoder layer + final RMSNorm over N sequences of S tokens, on the fp32 stream h->h
// ([N*S, D], already embedded).  rq: enc_request of the same E; the workspace holds plan_encoder_workspace of it.  kv_len_dev: per-sequence
// valid key count (rq.has_kv_len); out: [N*S, D] bf16; cache: rq.has_cache.  A refusal of the plan is ACE355_ERR_INVALID with its text.
int run_encoder_pass(EncBase* h, const EncoderW& E, const EncPassRequest& rq, const int* kv_len_dev, bf16_t* out, hipStream_t s,
                     const KvCache* cache = nullptr);
void free_encoder(EncBase* h);   // free_base + the workspace

// textenc.hip.  k_first_dev (null: none): per-sequence first visible key; query rows below it store zeros.
// Hq = 2 Hkv or 4 Hkv: q head hq reads kv head hq / (Hq / Hkv).
int launch_causal_attention(const bf16_t* qkv, int ld, int k_col0, int v_col0, bf16_t* out, int o_ld, int N, int S, int Hq, int Hkv,
                            float scale, hipStream_t s, const int* k_first_dev = nullptr);
int launch_embed_rows(const bf16_t* table, const int* ids_dev, float* out_f32, bf16_t* out_bf, long rows, int D, hipStream_t s);

// lm.hip.  Rows n * S + s of the QKV workspace -> layer `layer` of the cache at position pos0 + s.
int launch_kv_store(const bf16_t* qkv, int ld, int k_col0, int v_col0, const KvCache& c, int layer, int N, int S, int Hkv, int pos0,
                    hipStream_t s);
// One query row per (sequence, q head) (row n of the QKV workspace) over keys [first[n], len) of the cache; out [N, Hq * 128] bf16,
// Hq = 2 Hkv or 4 Hkv.
int launch_decode_attention(const bf16_t* qkv, int ld, const KvCache& c, int layer, int len, bf16_t* out, int N, int Hq, int Hkv,
                            float scale, hipStream_t s);

}  // namespace ace355
