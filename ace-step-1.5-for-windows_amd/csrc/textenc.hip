// textenc.hip - the caption text encoder behind ace355.h: transformers' Qwen3Model as the reference loads it
// (Qwen3-Embedding-0.6B, init_service_loader.py:146-161) = token embedding, num_layers pre-norm decoder layers with CAUSAL self-attention,
// final RMSNorm; and its embed_tokens row gather for the lyric ids (conditioning_embed.py:71-79).
//
// The decoder layer is the shared encoder stack (encoder.hip: run_encoder_pass, EncBase::causal) with two differences: the attention is
// causal (a kernel of its own below, causal_gqa_attn_kernel; attn.hip is untouched), and the input is a gather from the [vocab, hidden]
// table, not a Linear.  This file holds that kernel, the gather, the handle's two non-layer keys and create / encode / embed.
//
// No attention mask: the reference calls the encoder with right-padded ids and no mask, so the stack is purely causal over the padded
// length.  Valid rows never see the pads, and the pad rows attend the whole prefix and the earlier pads - their outputs reach the DiT
// (INTEGRATION.md 3b), so they are computed exactly like every other row.
#include <math.h>

#include <string>

#include "encoder.h"

using namespace ace355;

namespace {

// ------------------------------------------------------------------------------------------------ causal GQA attention
// out[n][s][hq*128 + d] = softmax_{j <= s}(scale q[n][s][hq] . k[n][j][hq/G]) v[n][j][hq/G], Hq = G Hkv with G = 2 (the text encoder, the
// 0.6B / 1.7B LMs) or 4 (the 4B LM), head dim 128.
// q / k / v are columns of the QKV GEMM's output rows (q and k in the head-pair dim order of PACK_ROWS_HEADPAIR - the dot product does
// not see a common permutation of the head dims -, v in natural order, so `out` is in natural order).
//
// One workgroup = 64 query rows of ONE q head pair hp (8 waves: wave w takes q head 2 hp + (w >> 2), rows 16 (w & 3) .. + 15) and the kv
// head hp >> pair_shift both heads read, so a K / V tile of 64 keys is staged in LDS once for 128 query rows.  With G = 2 a pair is a kv
// head (pair_shift 0); with G = 4 the two pairs of a kv head each stage its tiles: the kernel is bound by its MFMAs, not by K / V.
// Key tiles wholly above the diagonal are never visited
// (the query block and the key tile are both 64 wide: tiles 0 .. blockIdx.x); the per-element causal predicate runs on the diagonal tile
// only, where masked scores are -inf, so their probabilities are exactly 0.  Reads past the sequence end are clamped to row S - 1 (real,
// finite data whose probability is 0 for every stored row), rows >= S are not stored.  Everything else is fixed-order: bit-reproducible.
//
// FIRST (the LM's left-padded batches, lm.hip): sequence n sees keys k_first[n] <= j <= s only.  Key tiles wholly below k_first[n] are
// skipped, the tile that holds it gets a per-element predicate like the diagonal one, and a query row with no visible key (a pad row)
// has a running max of -inf throughout: its exponentials are taken against 0 instead, its row sum stays 0, and it stores zeros.  Without
// FIRST the kernel is the text encoder's, instruction for instruction.
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
    int S, pair_shift;  // kv head of q head pair hp = hp >> pair_shift
    float scale_log2;   // softmax scale * log2(e)
    const int* k_first; // FIRST only: [N]
};

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

template <bool FIRST>
__global__ __launch_bounds__(CA_THREADS) void causal_gqa_attn_kernel(CausalArgs a) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[CA_KB * CA_LDK];
    __shared__ __attribute__((aligned(16))) bf16_t Vt[128 * CA_LDV];
    const int qb = blockIdx.x, kvh = (int)blockIdx.y >> a.pair_shift, n = blockIdx.z;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, c = l & 15, g = l >> 4;
    const int S = a.S;
    const int hq = 2 * blockIdx.y + (w >> 2);
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
    int first = 0;
    if constexpr (FIRST) first = a.k_first[n];

    for (int kt = first / CA_KB; kt <= qb; ++kt) {
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
                if constexpr (FIRST) {
                    if (kt * CA_KB + mt * 16 + g * 4 + r < first) v = -INFINITY;
                }
                sc[mt][r] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float m_new = fmaxf(m_run, mx);   // finite: key 0 of tile 0 is visible to every query (FIRST: to every row that is not a pad)
        const float m_old = m_run;
        m_run = m_new;
        if constexpr (FIRST) m_new = m_new == -INFINITY ? 0.f : m_new;   // a pad row so far: exp2(-inf - 0) = 0, never -inf - -inf
        const float alpha = __builtin_amdgcn_exp2f(m_old - m_new);
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
    float inv = 1.0f / l_run;
    if constexpr (FIRST) inv = l_run > 0.f ? inv : 0.f;   // a pad row: zeros
    bf16_t* op = a.out + (row0 + q_abs) * a.o_ld + hq * 128 + g * 4;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
        *reinterpret_cast<uint2*>(op + dt * 16) = make_uint2(pack_bf2(o[dt][0] * inv, o[dt][1] * inv), pack_bf2(o[dt][2] * inv, o[dt][3] * inv));
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

}  // namespace

int ace355::launch_causal_attention(const bf16_t* qkv, int ld, int k_col0, int v_col0, bf16_t* out, int o_ld, int N, int S, int Hq, int Hkv,
                                    float scale, hipStream_t s, const int* k_first_dev) {
    ACE_CHECK(N > 0 && S > 0 && Hkv > 0 && N <= 65535 && Hkv <= 65535, "causal attention: sizes");
    ACE_CHECK(Hq == 2 * Hkv || Hq == 4 * Hkv, "causal attention: 2 or 4 q heads per kv head");
    ACE_CHECK(Hq / 2 <= 65535, "causal attention: sizes");
    ACE_CHECK(ld % 8 == 0 && k_col0 % 8 == 0 && v_col0 % 8 == 0 && o_ld % 4 == 0, "causal attention: 16-byte rows");
    CausalArgs a{qkv, ld, k_col0, v_col0, out, o_ld, S, Hq == 4 * Hkv ? 1 : 0, scale * 1.4426950408889634f, k_first_dev};
    const dim3 grid((S + CA_QB - 1) / CA_QB, Hq / 2, N);
    if (k_first_dev) hipLaunchKernelGGL(causal_gqa_attn_kernel<true>, grid, dim3(CA_THREADS), 0, s, a);
    else hipLaunchKernelGGL(causal_gqa_attn_kernel<false>, grid, dim3(CA_THREADS), 0, s, a);
    ACE_LAUNCH_CHECK();
    return 0;
}

int ace355::launch_embed_rows(const bf16_t* table, const int* ids_dev, float* out_f32, bf16_t* out_bf, long rows, int D, hipStream_t s) {
    ACE_CHECK(D % 8 == 0 && rows > 0 && rows <= 0x7fffffffL, "embed: sizes");
    hipLaunchKernelGGL(embed_rows_kernel, dim3((unsigned)rows), dim3(128), 0, s, table, ids_dev, out_f32, out_bf, D);
    ACE_LAUNCH_CHECK();
    return 0;
}

struct ace355_textenc : EncBase {
    ace355_textenc_config cfg;
    bf16_t* embed = nullptr;   // [vocab][D]
    EncoderW enc;              // layers / norm (no input Linear)
    int* ids_dev = nullptr;
    long ids_cap = 0;
};

namespace {

// Map a key of Qwen3Model.state_dict() to its packed destination.
bool tx_resolve(ace355_textenc* h, const std::string& name, PackDest* d) {
    const long D = h->D;
    if (name == "embed_tokens.weight") { *d = pack_rows(h->embed, 1, h->cfg.vocab_size, D, D, 0); return true; }
    if (name == "norm.weight") { *d = pack_rows(h->enc.norm, 0, 1, D, D, 0); return true; }
    return resolve_encoder_layers(*h, h->enc, name, 0, d);
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
    enc_init(h, cfg->hidden_size, cfg->intermediate_size, cfg->num_heads, cfg->num_kv_heads, 0, 0, cfg->rms_norm_eps, cfg->rope_theta);
    h->causal = true;
    int rc = dev_alloc(h->allocs, &h->embed, (size_t)cfg->vocab_size * h->D);
    if (!rc) rc = alloc_encoder(h, h->enc, cfg->num_layers, 0);
    if (rc) { ace355_textenc_destroy(h); return rc; }
    h->expected_tensors = 2 + (size_t)cfg->num_layers * 11;
    *out = h;
    return ACE355_OK;
}

void ace355_textenc_destroy(ace355_textenc* h) {
    if (!h) return;
    hipDeviceSynchronize();
    free_encoder(h);
    if (h->ids_dev) hipFree(h->ids_dev);
    delete h;
}

int ace355_textenc_load_tensor(ace355_textenc* h, const char* name, const void* data, int dtype, int64_t numel, int is_device) {
    ACE_CHECK(h && name && data, "textenc_load_tensor: null argument");
    ACE_CHECK(dtype == ACE355_DTYPE_F32 || dtype == ACE355_DTYPE_BF16, "textenc_load_tensor: dtype");
    PackDest d;
    if (!tx_resolve(h, name, &d)) return unknown_tensor("textenc_load_tensor", name);
    return load_packed(h, d, name, data, dtype, numel, is_device, "textenc_load_tensor");
}

int ace355_textenc_finalize(ace355_textenc* h) {
    ACE_CHECK(h, "textenc_finalize: null handle");
    return finalize_loaded(h, "textenc_finalize");
}

int ace355_textenc_encode(ace355_textenc* h, const int32_t* ids_host, int N, int S, void* out_dev, void* stream) {
    ACE_CHECK(h && ids_host && out_dev, "textenc_encode: null argument");
    if (!h->finalized) { set_error("textenc_encode: call ace355_textenc_finalize first"); return ACE355_ERR_STATE; }
    ACE_CHECK(N > 0 && S > 0 && N <= 65535 && (long)N * S <= ACE355_TEXTENC_MAX_TOKENS, "textenc_encode: sizes");
    hipStream_t s = (hipStream_t)stream;
    const long M = (long)N * S;
    const EncPassRequest rq = enc_request(*h, h->enc, N, S);
    int rc = tx_upload_ids(h, ids_host, M, "textenc_encode", s);
    if (!rc) rc = ensure_workspace(h, plan_encoder_workspace(&rq, 1, 0, 0), s);   // the five per-row buffers only: no V^T, no input Linear
    if (!rc) rc = launch_embed_rows(h->embed, h->ids_dev, h->h, nullptr, M, h->D, s);
    if (rc) return rc;
    return run_encoder_pass(h, h->enc, rq, nullptr, (bf16_t*)out_dev, s);
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
