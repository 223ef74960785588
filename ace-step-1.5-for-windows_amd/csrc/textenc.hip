// textenc.hip - the caption text encoder behind ace355.h: transformers' Qwen3Model as the reference loads it
// (Qwen3-Embedding-0.6B, init_service_loader.py:146-161) = token embedding, num_layers pre-norm decoder layers with CAUSAL self-attention,
// final RMSNorm; and its embed_tokens row gather for the lyric ids (conditioning_embed.py:71-79).
//
// The decoder layer is the condition encoder's (cond.hip: encoder_layers) with two differences: the attention is causal (a kernel of its
// own below, causal_gqa_attn_kernel; attn.hip is untouched), and the input is a gather from the [vocab, hidden] table, not a Linear.
// Every contraction and norm runs on the DiT's kernels (gemm.hip modes 4 / 2 / 3, elementwise.hip).
//
// No attention mask: the reference calls the encoder with right-padded ids and no mask, so the stack is purely causal over the padded
// length.  Valid rows never see the pads, and the pad rows attend the whole prefix and the earlier pads - their outputs reach the DiT
// (INTEGRATION.md 3b), so they are computed exactly like every other row.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <string>
#include <vector>

#include "../../include/ace355.h"
#include "common.h"

using namespace ace355;

namespace {

// ------------------------------------------------------------------------------------------------ causal GQA attention
// out[n][s][hq*128 + d] = softmax_{j <= s}(scale q[n][s][hq] . k[n][j][hq/2]) v[n][j][hq/2], Hq = 2 Hkv, head dim 128.
// q / k / v are columns of the QKV GEMM's output rows (q and k in the head-pair dim order of PACK_ROWS_HEADPAIR - the dot product does
// not see a common permutation of the head dims -, v in natural order, so `out` is in natural order).
//
// One workgroup = 64 query rows of ONE kv head and BOTH of its q heads (8 waves: wave w takes q head 2 kvh + (w >> 2), rows 16 (w & 3) ..
// + 15), so a K / V tile of 64 keys is staged in LDS once for 128 query rows.  Key tiles wholly above the diagonal are never visited
// (the query block and the key tile are both 64 wide: tiles 0 .. blockIdx.x); the per-element causal predicate runs on the diagonal tile
// only, where masked scores are -inf, so their probabilities are exactly 0.  Reads past the sequence end are clamped to row S - 1 (real,
// finite data whose probability is 0 for every stored row), rows >= S are not stored.  Everything else is fixed-order: bit-reproducible.
//
// MFMA 16x16x32 bf16 on transposed problems, so that the score accumulator IS the B operand of the PV product with no lane movement:
//   S^T[key][q] = K Q^T:   A = K rows (lane l: key l&15, dims 8(l>>4) .. + 7 of a 32-dim chunk), B = Q rows (q l&15, the same dims)
//                          C: lane l, reg r = S^T[key 4(l>>4) + r][q l&15]
//   O^T[d][q] += V^T P^T:  the 32 keys of a PV step are the two 16-key score blocks 2j, 2j+1, in the order the accumulators hold them:
//                          element e of lane l is key 16 (2j + (e>>2)) + 4 (l>>4) + (e&3) for both operands (A = V^T from LDS, B = P^T).
// The online softmax runs per query column (lane l&15): max / sum over the 4 registers, the 4 key blocks and the 4 lane groups.
constexpr int CA_QB = 64, CA_KB = 64, CA_THREADS = 512;
constexpr int CA_LDK = 128 + 8;    // K tile row pitch (bf16)
constexpr int CA_LDV = CA_KB + 8;  // V^T tile row pitch (bf16)

struct CausalArgs {
    const bf16_t* qkv;  // rows n * S + s of the QKV GEMM, row stride ld
    int ld, k_col0, v_col0;
    bf16_t* out;        // rows n * S + s, row stride o_ld
    int o_ld;
    int S, Hkv;
    float scale_log2;   // softmax scale * log2(e)
};

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__global__ __launch_bounds__(CA_THREADS) void causal_gqa_attn_kernel(CausalArgs a) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[CA_KB * CA_LDK];
    __shared__ __attribute__((aligned(16))) bf16_t Vt[128 * CA_LDV];
    const int qb = blockIdx.x, kvh = blockIdx.y, n = blockIdx.z;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, c = l & 15, g = l >> 4;
    const int S = a.S;
    const int hq = 2 * kvh + (w >> 2);
    const int q_abs = qb * CA_QB + (w & 3) * 16 + c;   // this lane's query column
    const long row0 = (long)n * S;

    bf16x8 qf[4];
    {
        const bf16_t* qp = a.qkv + (row0 + min(q_abs, S - 1)) * a.ld + hq * 128 + g * 8;
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) qf[kc] = as_bf16x8(ldg16(qp + kc * 32));
    }
    f32x4 o[8];
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    for (int kt = 0; kt <= qb; ++kt) {
        __syncthreads();   // the previous tile's LDS reads are done
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + i * CA_THREADS, key = idx >> 4, ch = idx & 15;
            const long r = row0 + min(kt * CA_KB + key, S - 1);
            const uint4 kv = ldg16(a.qkv + r * a.ld + a.k_col0 + kvh * 128 + ch * 8);
            *reinterpret_cast<uint4*>(&Ks[key * CA_LDK + ch * 8]) = kv;
            const uint4 vv = ldg16(a.qkv + r * a.ld + a.v_col0 + kvh * 128 + ch * 8);
            const uint32_t vw[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                Vt[(ch * 8 + 2 * e) * CA_LDV + key] = (bf16_t)(vw[e] & 0xffffu);
                Vt[(ch * 8 + 2 * e + 1) * CA_LDV + key] = (bf16_t)(vw[e] >> 16);
            }
        }
        __syncthreads();

        f32x4 sc[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            sc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) {
                const bf16x8 kf = as_bf16x8(*reinterpret_cast<const uint4*>(&Ks[(mt * 16 + c) * CA_LDK + kc * 32 + g * 8]));
                sc[mt] = mfma16(kf, qf[kc], sc[mt]);
            }
        }
        const bool diag = kt == qb;
        float mx = -INFINITY;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = sc[mt][r] * a.scale_log2;
                if (diag && kt * CA_KB + mt * 16 + g * 4 + r > q_abs) v = -INFINITY;
                sc[mt][r] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);   // finite: key 0 of tile 0 is visible to every query
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        float ps = 0.f;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(sc[mt][r] - m_new);
                sc[mt][r] = p;
                ps += p;
            }
        l_run = l_run * alpha + ps;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) o[dt] *= alpha;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint4 pu = make_uint4(pack_bf2(sc[2 * j][0], sc[2 * j][1]), pack_bf2(sc[2 * j][2], sc[2 * j][3]),
                                        pack_bf2(sc[2 * j + 1][0], sc[2 * j + 1][1]), pack_bf2(sc[2 * j + 1][2], sc[2 * j + 1][3]));
            const bf16x8 pb = as_bf16x8(pu);
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) {
                const bf16_t* vr = &Vt[(dt * 16 + c) * CA_LDV + 32 * j + g * 4];
                const uint2 lo = *reinterpret_cast<const uint2*>(vr);
                const uint2 hi = *reinterpret_cast<const uint2*>(vr + 16);
                o[dt] = mfma16(as_bf16x8(make_uint4(lo.x, lo.y, hi.x, hi.y)), pb, o[dt]);
            }
        }
    }
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    if (q_abs >= S) return;
    const float inv = 1.0f / l_run;
    bf16_t* op = a.out + (row0 + q_abs) * a.o_ld + hq * 128 + g * 4;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
        *reinterpret_cast<uint2*>(op + dt * 16) = make_uint2(pack_bf2(o[dt][0] * inv, o[dt][1] * inv), pack_bf2(o[dt][2] * inv, o[dt][3] * inv));
}

int launch_causal_attention(const bf16_t* qkv, int ld, int k_col0, int v_col0, bf16_t* out, int o_ld, int N, int S, int Hkv, float scale,
                            hipStream_t s) {
    ACE_CHECK(N > 0 && S > 0 && Hkv > 0 && N <= 65535 && Hkv <= 65535, "causal attention: sizes");
    ACE_CHECK(ld % 8 == 0 && k_col0 % 8 == 0 && v_col0 % 8 == 0 && o_ld % 4 == 0, "causal attention: 16-byte rows");
    CausalArgs a{qkv, ld, k_col0, v_col0, out, o_ld, S, Hkv, scale * 1.4426950408889634f};
    hipLaunchKernelGGL(causal_gqa_attn_kernel, dim3((S + CA_QB - 1) / CA_QB, Hkv, N), dim3(CA_THREADS), 0, s, a);
    ACE_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------ embedding gather
// row m of the output = row ids[m] of the bf16 table [vocab, D]: as fp32 (the encoder's residual stream) or as bf16 (embed_tokens).
// The ids were range-checked on the host.  D % 8 == 0: one 16-byte load per thread and step.
__global__ __launch_bounds__(128) void embed_rows_kernel(const bf16_t* __restrict__ table, const int* __restrict__ ids, float* out_f32,
                                                         bf16_t* out_bf, int D) {
    const long m = blockIdx.x;
    const bf16_t* src = table + (long)ids[m] * D;
    for (int col = threadIdx.x * 8; col < D; col += 128 * 8) {
        const uint4 v = ldg16(src + col);
        if (out_bf) {
            *reinterpret_cast<uint4*>(out_bf + m * D + col) = v;
        } else {
            float4* o = reinterpret_cast<float4*>(out_f32 + m * D + col);
            o[0] = make_float4(bf_lo(v.x), bf_hi(v.x), bf_lo(v.y), bf_hi(v.y));
            o[1] = make_float4(bf_lo(v.z), bf_hi(v.z), bf_lo(v.w), bf_hi(v.w));
        }
    }
}

int launch_embed_rows(const bf16_t* table, const int* ids_dev, float* out_f32, bf16_t* out_bf, long rows, int D, hipStream_t s) {
    ACE_CHECK(D % 8 == 0 && rows > 0 && rows <= 0x7fffffffL, "embed: sizes");
    hipLaunchKernelGGL(embed_rows_kernel, dim3((unsigned)rows), dim3(128), 0, s, table, ids_dev, out_f32, out_bf, D);
    ACE_LAUNCH_CHECK();
    return 0;
}

struct TxLayerW {
    bf16_t *wqkv, *wo, *wgu, *wdown;
    float *n_in, *n_post, *qn, *kn;
};

template <typename T>
int tx_alloc(std::vector<void*>& bag, T** p, size_t n) {
    void* q = nullptr;
    ACE_HIP(hipMalloc(&q, n * sizeof(T) + 256));
    bag.push_back(q);
    *p = reinterpret_cast<T*>(q);
    return 0;
}
#define TX_ALLOC(bag, ptr, n)                  \
    do {                                       \
        int _rc = tx_alloc(bag, &(ptr), (n));  \
        if (_rc) return _rc;                   \
    } while (0)

}  // namespace

struct ace355_textenc {
    ace355_textenc_config cfg;
    int D = 0, F = 0, QD = 0, KVD = 0, HQ = 0, KVH = 0;
    bf16_t* embed = nullptr;   // [vocab][D]
    float* norm = nullptr;
    std::vector<TxLayerW> layers;
    std::set<std::string> loaded;
    size_t expected_tensors = 0;
    bool finalized = false;
    std::vector<void*> allocs;
    void* stage = nullptr;
    size_t stage_bytes = 0;
    // workspace, sized for the largest call so far
    long ws_rows = 0;
    std::vector<void*> ws_allocs;
    float* h = nullptr;
    bf16_t *xn = nullptr, *qkv = nullptr, *ao = nullptr, *act = nullptr;
    int* ids_dev = nullptr;
    long ids_cap = 0;
    float *rope_cos = nullptr, *rope_sin = nullptr;
    int rope_S = 0;
    int* sk_cnt = nullptr;
};

namespace {

struct TxDest {
    void* dst;
    int is_bf16, mode;
    long rows, cols, dst_row0;
    int p0;
};

// Map a key of Qwen3Model.state_dict() to its packed destination (same packing as cond.hip's encoder layers).
bool tx_resolve(ace355_textenc* h, const std::string& name, TxDest* d) {
    const long D = h->D, F = h->F, QD = h->QD, KVD = h->KVD;
    auto rows = [&](void* dst, int bf, long r, long c, long row0) {
        *d = TxDest{dst, bf, PACK_ROWS, r, c, row0, 0};
        return true;
    };
    if (name == "embed_tokens.weight") return rows(h->embed, 1, h->cfg.vocab_size, D, 0);
    if (name == "norm.weight") return rows(h->norm, 0, 1, D, 0);
    if (name.rfind("layers.", 0) != 0) return false;
    const size_t dot = name.find('.', 7);
    if (dot == std::string::npos || dot == 7) return false;
    const std::string idx = name.substr(7, dot - 7);
    if (idx.find_first_not_of("0123456789") != std::string::npos) return false;
    const int li = atoi(idx.c_str());
    if (li < 0 || li >= (int)h->layers.size()) return false;
    TxLayerW& L = h->layers[li];
    const std::string q = name.substr(dot + 1);
    if (q == "input_layernorm.weight") return rows(L.n_in, 0, 1, D, 0);
    if (q == "post_attention_layernorm.weight") return rows(L.n_post, 0, 1, D, 0);
    if (q == "self_attn.q_proj.weight") { *d = TxDest{L.wqkv, 1, PACK_ROWS_HEADPAIR, QD, D, 0, 0}; return true; }
    if (q == "self_attn.k_proj.weight") { *d = TxDest{L.wqkv, 1, PACK_ROWS_HEADPAIR, KVD, D, QD, 0}; return true; }
    if (q == "self_attn.v_proj.weight") return rows(L.wqkv, 1, KVD, D, QD + KVD);
    if (q == "self_attn.o_proj.weight") return rows(L.wo, 1, D, QD, 0);
    if (q == "self_attn.q_norm.weight") return rows(L.qn, 0, 1, 128, 0);
    if (q == "self_attn.k_norm.weight") return rows(L.kn, 0, 1, 128, 0);
    if (q == "mlp.gate_proj.weight") { *d = TxDest{L.wgu, 1, PACK_ROWS_IL32, F, D, 0, 0}; return true; }
    if (q == "mlp.up_proj.weight") { *d = TxDest{L.wgu, 1, PACK_ROWS_IL32, F, D, 0, 1}; return true; }
    if (q == "mlp.down_proj.weight") return rows(L.wdown, 1, D, F, 0);
    return false;
}

int tx_ensure_rope(ace355_textenc* h, int S, hipStream_t s) {
    if (S <= h->rope_S) return 0;
    int cap = 512;
    while (cap < S) cap *= 2;
    TX_ALLOC(h->allocs, h->rope_cos, (size_t)cap * 64);
    TX_ALLOC(h->allocs, h->rope_sin, (size_t)cap * 64);
    int rc = launch_rope_table(h->rope_cos, h->rope_sin, cap, h->cfg.rope_theta, s);
    if (rc) return rc;
    h->rope_S = cap;
    if (!h->sk_cnt) {
        TX_ALLOC(h->allocs, h->sk_cnt, SK_CNT_INTS);
        ACE_HIP(hipMemsetAsync(h->sk_cnt, 0, SK_CNT_INTS * sizeof(int), s));
        if (int prc = gemm_verify_splitk_placement()) return prc;
    }
    return 0;
}

int tx_ensure_workspace(ace355_textenc* h, long rows, hipStream_t s) {
    if (rows <= h->ws_rows) return 0;
    ACE_HIP(hipStreamSynchronize(s));
    for (void* p : h->ws_allocs) hipFree(p);
    h->ws_allocs.clear();
    h->ws_rows = 0;
    const long R = rows, D = h->D, QKV = h->QD + 2 * h->KVD;
    TX_ALLOC(h->ws_allocs, h->h, (size_t)R * D);
    TX_ALLOC(h->ws_allocs, h->xn, (size_t)R * D);
    TX_ALLOC(h->ws_allocs, h->qkv, (size_t)(R + 64) * QKV);  // +64 rows: the last K tile's DMA rows are clamped, not skipped
    TX_ALLOC(h->ws_allocs, h->ao, (size_t)R * h->QD);
    TX_ALLOC(h->ws_allocs, h->act, (size_t)R * h->F);
    h->ws_rows = R;
    return 0;
}

// Host ids -> range check -> the handle's device buffer (the caller's array may be reused as soon as this returns).
int tx_upload_ids(ace355_textenc* h, const int32_t* ids, long n, const char* who, hipStream_t s) {
    for (long i = 0; i < n; ++i) {
        if (ids[i] < 0 || ids[i] >= h->cfg.vocab_size) {
            set_error(std::string(who) + ": token id " + std::to_string(ids[i]) + " at position " + std::to_string(i) +
                      " outside [0, " + std::to_string(h->cfg.vocab_size) + ")");
            return ACE355_ERR_INVALID;
        }
    }
    if (n > h->ids_cap) {
        ACE_HIP(hipStreamSynchronize(s));
        if (h->ids_dev) hipFree(h->ids_dev);
        h->ids_dev = nullptr;
        h->ids_cap = 0;
        ACE_HIP(hipMalloc((void**)&h->ids_dev, sizeof(int) * n + 256));
        h->ids_cap = n;
    }
    ACE_HIP(hipMemcpyAsync(h->ids_dev, ids, sizeof(int) * n, hipMemcpyHostToDevice, s));
    ACE_HIP(hipStreamSynchronize(s));   // `ids` is caller memory
    return 0;
}

}  // namespace

extern "C" {

int ace355_textenc_create(const ace355_textenc_config* cfg, ace355_textenc** out) {
    ACE_CHECK(cfg && out, "textenc_create: null argument");
    if (cfg->head_dim != 128 || cfg->num_kv_heads <= 0 || cfg->num_heads != 2 * cfg->num_kv_heads) {
        set_error("textenc_create: only head_dim 128 with num_heads == 2 * num_kv_heads is supported");
        return ACE355_ERR_UNSUPPORTED;
    }
    ACE_CHECK(cfg->hidden_size > 0 && cfg->hidden_size % 256 == 0 && cfg->intermediate_size > 0 && cfg->intermediate_size % 64 == 0,
              "textenc_create: hidden/intermediate size");
    ACE_CHECK(cfg->num_layers >= 0 && cfg->num_layers <= 256 && cfg->vocab_size > 0, "textenc_create: layer count / vocabulary");
    ace355_textenc* h = new ace355_textenc();
    h->cfg = *cfg;
    h->D = cfg->hidden_size; h->F = cfg->intermediate_size; h->HQ = cfg->num_heads; h->KVH = cfg->num_kv_heads;
    h->QD = cfg->num_heads * 128; h->KVD = cfg->num_kv_heads * 128;
    const size_t D = h->D, F = h->F, QD = h->QD, KVD = h->KVD;
    auto alloc_all = [&]() -> int {
        TX_ALLOC(h->allocs, h->embed, (size_t)cfg->vocab_size * D);
        TX_ALLOC(h->allocs, h->norm, D);
        h->layers.resize(cfg->num_layers);
        for (TxLayerW& L : h->layers) {
            TX_ALLOC(h->allocs, L.wqkv, (QD + 2 * KVD) * D);
            TX_ALLOC(h->allocs, L.wo, D * QD);
            TX_ALLOC(h->allocs, L.wgu, 2 * F * D);
            TX_ALLOC(h->allocs, L.wdown, D * F);
            TX_ALLOC(h->allocs, L.n_in, D);
            TX_ALLOC(h->allocs, L.n_post, D);
            TX_ALLOC(h->allocs, L.qn, 128);
            TX_ALLOC(h->allocs, L.kn, 128);
        }
        return 0;
    };
    if (int rc = alloc_all()) { ace355_textenc_destroy(h); return rc; }
    h->expected_tensors = 2 + (size_t)cfg->num_layers * 11;
    *out = h;
    return ACE355_OK;
}

void ace355_textenc_destroy(ace355_textenc* h) {
    if (!h) return;
    hipDeviceSynchronize();
    for (void* p : h->allocs) hipFree(p);
    for (void* p : h->ws_allocs) hipFree(p);
    if (h->ids_dev) hipFree(h->ids_dev);
    if (h->stage) hipFree(h->stage);
    delete h;
}

int ace355_textenc_load_tensor(ace355_textenc* h, const char* name, const void* data, int dtype, int64_t numel, int is_device) {
    ACE_CHECK(h && name && data, "textenc_load_tensor: null argument");
    ACE_CHECK(dtype == ACE355_DTYPE_F32 || dtype == ACE355_DTYPE_BF16, "textenc_load_tensor: dtype");
    TxDest d;
    if (!tx_resolve(h, name, &d)) {
        set_error(std::string("textenc_load_tensor: unknown tensor name '") + name + "'");
        return ACE355_ERR_INVALID;
    }
    if (numel != d.rows * d.cols) {
        set_error(std::string("textenc_load_tensor: wrong element count for '") + name + "': got " + std::to_string(numel) +
                  ", expected " + std::to_string(d.rows * d.cols));
        return ACE355_ERR_INVALID;
    }
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
    int rc = launch_pack(src, dtype, d.dst, d.is_bf16, d.mode, d.rows, d.cols, d.cols, d.dst_row0, d.p0, 0, nullptr);
    if (rc) return rc;
    ACE_HIP(hipDeviceSynchronize());
    h->loaded.insert(name);
    h->finalized = false;
    return ACE355_OK;
}

int ace355_textenc_finalize(ace355_textenc* h) {
    ACE_CHECK(h, "textenc_finalize: null handle");
    if (h->loaded.size() != h->expected_tensors) {
        set_error("textenc_finalize: " + std::to_string(h->loaded.size()) + " of " + std::to_string(h->expected_tensors) + " tensors loaded");
        return ACE355_ERR_STATE;
    }
    if (h->stage) { hipFree(h->stage); h->stage = nullptr; h->stage_bytes = 0; }
    h->finalized = true;
    return ACE355_OK;
}

int ace355_textenc_encode(ace355_textenc* h, const int32_t* ids_host, int N, int S, void* out_dev, void* stream) {
    ACE_CHECK(h && ids_host && out_dev, "textenc_encode: null argument");
    if (!h->finalized) { set_error("textenc_encode: call ace355_textenc_finalize first"); return ACE355_ERR_STATE; }
    ACE_CHECK(N > 0 && S > 0 && N <= 65535 && (long)N * S <= ACE355_TEXTENC_MAX_TOKENS, "textenc_encode: sizes");
    hipStream_t s = (hipStream_t)stream;
    const int M = N * S, D = h->D, F = h->F, QD = h->QD, KVD = h->KVD, QKV = QD + 2 * KVD;
    const float eps = h->cfg.rms_norm_eps;
    int rc = tx_upload_ids(h, ids_host, M, "textenc_encode", s);
    if (!rc) rc = tx_ensure_workspace(h, M, s);
    if (!rc) rc = tx_ensure_rope(h, S, s);
    if (!rc) rc = launch_embed_rows(h->embed, h->ids_dev, h->h, nullptr, M, D, s);
    if (rc) return rc;
    GemmEpilogue ep{};
    for (const TxLayerW& W : h->layers) {
        // self attention: norm, QKV with q / k head-norm + RoPE in the epilogue, causal attention, h += o_proj
        rc = launch_rmsnorm_mod(h->h, W.n_in, h->xn, M, D, eps, nullptr, nullptr, nullptr, nullptr, 0, S, s);
        if (rc) return rc;
        ep = GemmEpilogue{4, nullptr, nullptr, nullptr, 0, S};
        ep.hn_wq = W.qn, ep.hn_wk = W.kn, ep.hn_cos = h->rope_cos, ep.hn_sin = h->rope_sin;
        ep.hn_q_cols = QD, ep.hn_qk_cols = QD + KVD, ep.hn_eps = eps;
        rc = launch_gemm(h->xn, D, W.wqkv, D, h->qkv, QKV, M, QKV, D, ep, s);
        if (rc) return rc;
        rc = launch_causal_attention(h->qkv, QKV, QD, QD + KVD, h->ao, QD, N, S, h->KVH, 1.0f / sqrtf(128.0f), s);
        if (rc) return rc;
        ep = GemmEpilogue{2, nullptr, nullptr, nullptr, 0, S};
        ep.sk_cnt = h->sk_cnt;
        rc = launch_gemm(h->ao, QD, W.wo, QD, h->h, D, M, D, QD, ep, s);
        if (rc) return rc;
        // SwiGLU MLP
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
    return launch_rmsnorm_mod(h->h, h->norm, (bf16_t*)out_dev, M, D, eps, nullptr, nullptr, nullptr, nullptr, 0, S, s);
}

int ace355_textenc_embed(ace355_textenc* h, const int32_t* ids_host, int64_t n, void* out_dev, void* stream) {
    ACE_CHECK(h && ids_host && out_dev, "textenc_embed: null argument");
    if (!h->finalized) { set_error("textenc_embed: call ace355_textenc_finalize first"); return ACE355_ERR_STATE; }
    ACE_CHECK(n > 0 && n <= ACE355_TEXTENC_MAX_TOKENS, "textenc_embed: sizes");
    ACE_CHECK(((uintptr_t)out_dev & 15) == 0, "textenc_embed: output must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    int rc = tx_upload_ids(h, ids_host, n, "textenc_embed", s);
    if (rc) return rc;
    return launch_embed_rows(h->embed, h->ids_dev, nullptr, (bf16_t*)out_dev, n, h->D, s);
}

}  // extern "C"
