// lm.hip - the 5 Hz LM's forward behind ace355.h: transformers' Qwen3ForCausalLM as LLMHandler._forward_pass calls
// it (llm_inference.py:416-438) = the text encoder's stack (encoder.hip: run_encoder_pass, causal) run in steps over a KV cache, and the LM
// head on the last column.  Prefill is the text encoder's pass with a per-sequence first visible key (textenc.hip, FIRST) plus the cache
// store; a decode step is the same layer code at M = N rows, S = 1, with the attention below reading the cache.
//
// This file holds the cache store, the cache fan-out, the decode attention with its merge, the LM head, and the handle (ace355_lm_score runs
// the prefill's pass and hands the final norm of the target rows to lm_score.hip).  The cut of a cache into chunks is
// lm_plan.h's, a function of the length alone.  No atomics in the forward: every result has one summation order, so the same calls give
// the same bits, and a sequence's bits do not depend on the other sequences of the batch.  (The one atomic of the file is an integer count
// of replaced ids in lm_tokens_kernel.)
#include <math.h>

#include <string>
#include <vector>

#include "encoder.h"
#include "lm_plan.h"

using namespace ace355;

namespace {

// ------------------------------------------------------------------------------------------------ KV store
// The K and V columns of QKV row n * S + s -> cache[K | V][n][kv head][pos0 + s][128]; one thread = one 16-byte piece.
__global__ __launch_bounds__(256) void kv_store_kernel(const bf16_t* __restrict__ qkv, int ld, int k_col0, int v_col0, bf16_t* __restrict__ kc,
                                                       bf16_t* __restrict__ vc, long seq_stride, int max_pos, int pos0, int S, int Hkv,
                                                       long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = (int)(idx & 15), is_v = (int)((idx >> 4) & 1);
    long t = idx >> 5;
    const int hk = (int)(t % Hkv);
    t /= Hkv;
    const int s = (int)(t % S);
    const long n = t / S;
    const uint4 v = ldg16(qkv + (n * S + s) * ld + (is_v ? v_col0 : k_col0) + hk * 128 + ch * 8);
    bf16_t* dst = (is_v ? vc : kc) + n * seq_stride + ((long)hk * max_pos + pos0 + s) * 128 + ch * 8;
    *reinterpret_cast<uint4*>(dst) = v;
}

// ------------------------------------------------------------------------------------------------ cache fan-out
// One wave of plan_lm_fan_out: copy c moves the K and V rows [0, len) of every layer and kv head from sequence src[c] to sequence
// dst[c] of the same cache.  The rows below first[src] go along: decode_attn_kernel walks whole rounds of 16 keys and a masked key
// still enters 0 x V, so every row < len of a held sequence must be a written, finite one - the source's stored pad rows are.
// One thread = one 16-byte piece; blockIdx.y = the copy, blockIdx.x walks (layer, K | V, kv head, row, piece) with the piece fastest,
// so a wavefront moves four whole rows.  No copy of a wave reads what another one of it writes (lm_plan.h), and a thread reads and
// writes different sequences, so there is nothing to order inside the launch.
struct FanOutArgs {
    bf16_t* kv;
    long slab, seq_stride;   // elements of one layer's K (or V) and of one sequence in it
    int max_pos, Hkv, planes, len, count;   // planes = layers x (K, V)
    int dst[LM_MAX_SEQS], src[LM_MAX_SEQS];
};

__global__ __launch_bounds__(256) void kv_fan_out_kernel(FanOutArgs a) {
    const int c = blockIdx.y;
    if (c >= a.count) return;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)a.planes * a.Hkv * a.len * 16) return;
    const int ch = (int)(idx & 15);
    long t = idx >> 4;
    const int pos = (int)(t % a.len);
    t /= a.len;
    const int hk = (int)(t % a.Hkv);
    const long plane = t / a.Hkv;
    const long off = plane * a.slab + ((long)hk * a.max_pos + pos) * 128 + ch * 8;
    *reinterpret_cast<uint4*>(a.kv + off + a.dst[c] * a.seq_stride) = ldg16(a.kv + off + a.src[c] * a.seq_stride);
}

// first[n] of the fanned-out sequences, by value: the host knows them, and a kernel argument needs no host buffer that outlives the call
struct FirstArgs { int first[LM_MAX_SEQS]; };
__global__ __launch_bounds__(64) void lm_set_first_kernel(FirstArgs a, int N, int* __restrict__ first) {
    if ((int)threadIdx.x < N) first[threadIdx.x] = a.first[threadIdx.x];
}

// ------------------------------------------------------------------------------------------------ decode attention
// One query row per (sequence, q head): out[n][hq] = softmax_{first[n] <= j < len}(scale q[n][hq] . K[n][hq/G][j]) V[n][hq/G][j].
//
// Bound by the K / V bytes, so VALU dot products: a workgroup takes one (chunk of keys, kv head, sequence) and ALL G q heads of that kv
// head (G = 2, or 4 for Qwen3-4B's 32 / 8 layout), and reads every K / V row of its chunk once.  256 threads = 16 key groups x 16 lanes; a lane holds 8 of the 128 head dims
// (one 16-byte load per row), a key group walks the chunk's keys kg, kg + 16, ... with its own online softmax (running max, row sum and
// un-normalised O for each head).  The 16 groups are then merged through LDS in group order, and the workgroup leaves un-normalised
// fp32 O, the max and the row sum of its chunk; decode_merge_kernel combines a sequence's chunks in chunk order, as attn.hip's kv_split
// merge does.  Keys outside [first, len) get -inf; a group or a chunk without a visible key carries max -inf / sum 0 and is skipped by
// the merges, so no exponential is ever taken of -inf - -inf.
struct DecodeArgs {
    const bf16_t* qkv;   // row n: this step's q heads (head-normed, rotated), row stride ld
    int ld;
    const bf16_t *kc, *vc;   // this layer's K / V: [n][kv head][max_pos][128]
    long seq_stride;
    int max_pos;
    const int* first;
    int len, chunk, Hkv;
    float scale_log2;
    float *part_o, *part_ml;   // [n][hq][LM_MAX_SPLITS][128], [..][2]
};

__device__ __forceinline__ void unpack8(uint4 v, float* f) {
    f[0] = bf_lo(v.x); f[1] = bf_hi(v.x); f[2] = bf_lo(v.y); f[3] = bf_hi(v.y);
    f[4] = bf_lo(v.z); f[5] = bf_hi(v.z); f[6] = bf_lo(v.w); f[7] = bf_hi(v.w);
}

template <int G>   // q heads per kv head: 2 or 4
__global__ __launch_bounds__(256) void decode_attn_kernel(DecodeArgs a) {
    constexpr int KG = LM_DECODE_KEY_GROUPS;
    __shared__ float go[KG][G][128];
    __shared__ float gm[G][KG], gl[G][KG];
    const int c = blockIdx.x, kvh = blockIdx.y, n = blockIdx.z;
    const int tid = threadIdx.x, kg = tid >> 4, dc = tid & 15;
    const int first = a.first[n];
    const int k_lo = c * a.chunk, k_hi = min(a.len, k_lo + a.chunk);
    const int Hq = G * a.Hkv;
    const long pbase = ((long)n * Hq + G * kvh) * LM_MAX_SPLITS + c;   // head G kvh; head G kvh + h is h LM_MAX_SPLITS further on

    float q[G][8];
#pragma unroll
    for (int h = 0; h < G; ++h) unpack8(ldg16(a.qkv + (long)n * a.ld + (G * kvh + h) * 128 + dc * 8), q[h]);
    float m[G], l[G], o[G][8];
#pragma unroll
    for (int h = 0; h < G; ++h) {
        m[h] = -INFINITY;
        l[h] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[h][e] = 0.f;
    }

    const bf16_t* kb = a.kc + n * a.seq_stride + (long)kvh * a.max_pos * 128 + dc * 8;
    const bf16_t* vb = a.vc + n * a.seq_stride + (long)kvh * a.max_pos * 128 + dc * 8;
    // rounds of 16 keys that hold a visible one (uniform over the workgroup; a skipped round would have changed nothing)
    const int r_lo = first > k_lo ? (first - k_lo) / KG : 0, r_hi = (k_hi - k_lo + KG - 1) / KG;
    for (int r = r_lo; r < r_hi; ++r) {
        const int key = k_lo + r * KG + kg;
        const long row = (long)min(key, a.len - 1) * 128;   // (rows < len are written; a clamped key is masked)
        float kf[8], vf[8];
        unpack8(ldg16(kb + row), kf);
        unpack8(ldg16(vb + row), vf);
        float s[G];
#pragma unroll
        for (int h = 0; h < G; ++h) {
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) d += q[h][e] * kf[e];
#pragma unroll
            for (int x = 8; x > 0; x >>= 1) d += __shfl_xor(d, x, 64);   // over the key group's 16 lanes: every lane the same bits
            s[h] = d * a.scale_log2;
        }
        const bool visible = key >= first && key < k_hi;
#pragma unroll
        for (int h = 0; h < G; ++h) {
            const float sv = visible ? s[h] : -INFINITY;
            const float m_new = fmaxf(m[h], sv);
            const bool any = m_new > -INFINITY;
            const float alpha = any ? __builtin_amdgcn_exp2f(m[h] - m_new) : 1.f;
            const float p = any ? __builtin_amdgcn_exp2f(sv - m_new) : 0.f;
            m[h] = m_new;
            l[h] = l[h] * alpha + p;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[h][e] = o[h][e] * alpha + p * vf[e];
        }
    }
#pragma unroll
    for (int h = 0; h < G; ++h) {
#pragma unroll
        for (int e = 0; e < 8; ++e) go[kg][h][dc * 8 + e] = o[h][e];
        if (dc == 0) { gm[h][kg] = m[h]; gl[h][kg] = l[h]; }
    }
    __syncthreads();
    // thread -> (head of a pair, dim); one pass per head pair, the 16 groups in group order
    const int d = tid & 127;
#pragma unroll
    for (int hp = 0; hp < G / 2; ++hp) {
        const int h = 2 * hp + (tid >> 7);
        float M = -INFINITY;
#pragma unroll
        for (int g = 0; g < KG; ++g) M = fmaxf(M, gm[h][g]);
        float acc = 0.f, L = 0.f;
        if (M > -INFINITY) {
#pragma unroll
            for (int g = 0; g < KG; ++g) {
                const float w = gm[h][g] > -INFINITY ? __builtin_amdgcn_exp2f(gm[h][g] - M) : 0.f;
                acc += w * go[g][h][d];
                L += w * gl[h][g];
            }
        }
        const long p = pbase + (long)h * LM_MAX_SPLITS;
        a.part_o[p * 128 + d] = acc;
        if (d == 0) { a.part_ml[p * 2] = M; a.part_ml[p * 2 + 1] = L; }
    }
}

// out[n][hq][2t, 2t + 1] from the chunks' partials, in chunk order.  (Every sequence has a visible key - first < P <= len - so L > 0;
// the guard only keeps a broken invariant from becoming a NaN.)
__global__ __launch_bounds__(64) void decode_merge_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml, int splits,
                                                          bf16_t* __restrict__ out, int o_ld) {
    const int hq = blockIdx.x, n = blockIdx.y, t = threadIdx.x;
    const long base = ((long)n * gridDim.x + hq) * LM_MAX_SPLITS;
    float M = -INFINITY;
    for (int c = 0; c < splits; ++c) M = fmaxf(M, part_ml[(base + c) * 2]);
    float a0 = 0.f, a1 = 0.f, L = 0.f;
    for (int c = 0; c < splits; ++c) {
        const float mc = part_ml[(base + c) * 2];
        if (!(mc > -INFINITY)) continue;
        const float w = __builtin_amdgcn_exp2f(mc - M);
        const float2 o = *reinterpret_cast<const float2*>(part_o + (base + c) * 128 + 2 * t);
        a0 += w * o.x;
        a1 += w * o.y;
        L += w * part_ml[(base + c) * 2 + 1];
    }
    const float inv = L > 0.f ? 1.0f / L : 0.f;
    *reinterpret_cast<uint32_t*>(out + (long)n * o_ld + hq * 128 + 2 * t) = pack_bf2(a0 * inv, a1 * inv);
}

// ------------------------------------------------------------------------------------------------ LM head
// logits[m][v] = sum_k x[m][k] W[v][k]: x = Mr <= 16 bf16 rows (row stride x_stride: the last column of every sequence, read where the
// final norm left it), W bf16 [V, D], fp32 accumulators and fp32 out [Mr, V].  One wave per vocabulary row, all rows of x at once, so W
// is streamed exactly once per call; V needs no padding.  The shape of elementwise.hip's small_linear_kernel, with bf16 strided input.
template <int MT>
__global__ __launch_bounds__(256) void lm_head_kernel(const bf16_t* __restrict__ x, long x_stride, const bf16_t* __restrict__ W,
                                                      float* __restrict__ out, int Mr, int V, int D) {
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= V) return;
    float acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = 0.f;
    const bf16_t* wr = W + (long)v * D;
    for (int k0 = lane * 8; k0 < D; k0 += 512) {
        float wf[8];
        unpack8(ldg16(wr + k0), wf);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < Mr) {
                float xf[8];
                unpack8(ldg16(x + m * x_stride + k0), xf);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[m] += wf[e] * xf[e];
            }
        }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = wave_sum(acc[m]);
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
            if (m < Mr) out[(long)m * V + v] = acc[m];
    }
}

int launch_lm_head(const bf16_t* x, long x_stride, const bf16_t* W, float* out, int Mr, int V, int D, hipStream_t s) {
    ACE_CHECK(Mr > 0 && Mr <= LM_MAX_SEQS && V > 0 && D % 8 == 0 && x_stride % 8 == 0, "lm head: sizes");
    hipLaunchKernelGGL(lm_head_kernel<LM_MAX_SEQS>, dim3((V + 3) / 4), dim3(256), 0, s, x, x_stride, W, out, Mr, V, D);
    ACE_LAUNCH_CHECK();
    return 0;
}

}  // namespace

int ace355::launch_kv_store(const bf16_t* qkv, int ld, int k_col0, int v_col0, const KvCache& c, int layer, int N, int S, int Hkv, int pos0,
                            hipStream_t s) {
    ACE_CHECK(c.kv && N > 0 && N <= c.max_seqs && S > 0 && pos0 >= 0 && pos0 + S <= c.max_pos && layer >= 0, "kv store: cache bounds");
    ACE_CHECK(ld % 8 == 0 && k_col0 % 8 == 0 && v_col0 % 8 == 0, "kv store: 16-byte rows");
    const long slab = c.slab(Hkv), total = (long)N * S * Hkv * 32;
    bf16_t* kc = c.kv + (long)layer * 2 * slab;
    hipLaunchKernelGGL(kv_store_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, qkv, ld, k_col0, v_col0, kc, kc + slab,
                       (long)Hkv * c.max_pos * 128, c.max_pos, pos0, S, Hkv, total);
    ACE_LAUNCH_CHECK();
    return 0;
}

int ace355::launch_decode_attention(const bf16_t* qkv, int ld, const KvCache& c, int layer, int len, bf16_t* out, int N, int Hq, int Hkv,
                                    float scale, hipStream_t s) {
    ACE_CHECK(c.kv && c.first_dev && c.part_o && c.part_ml && N > 0 && N <= c.max_seqs && Hkv > 0 && len > 0 && len <= c.max_pos &&
                  layer >= 0, "decode attention: cache bounds");
    ACE_CHECK(ld % 8 == 0, "decode attention: 16-byte rows");
    ACE_CHECK(Hq == 2 * Hkv || Hq == 4 * Hkv, "decode attention: 2 or 4 q heads per kv head");
    const LmDecodePlan p = plan_lm_decode(len);
    ACE_CHECK(p.splits >= 1 && p.splits <= LM_MAX_SPLITS && p.chunk % LM_DECODE_KEY_GROUPS == 0, "decode attention: plan");
    const long slab = c.slab(Hkv);
    const bf16_t* kc = c.kv + (long)layer * 2 * slab;
    DecodeArgs a{qkv, ld, kc, kc + slab, (long)Hkv * c.max_pos * 128, c.max_pos, c.first_dev, len, p.chunk, Hkv,
                 scale * 1.4426950408889634f, c.part_o, c.part_ml};
    if (Hq == 2 * Hkv) hipLaunchKernelGGL(decode_attn_kernel<2>, dim3(p.splits, Hkv, N), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(decode_attn_kernel<4>, dim3(p.splits, Hkv, N), dim3(256), 0, s, a);
    ACE_LAUNCH_CHECK();
    hipLaunchKernelGGL(decode_merge_kernel, dim3(Hq, N), dim3(64), 0, s, c.part_o, c.part_ml, p.splits, out, Hq * 128);
    ACE_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------ the handle
struct ace355_lm : EncBase {
    ace355_lm_config cfg;
    bf16_t* embed = nullptr;   // [vocab][D]
    bf16_t* head = nullptr;    // [vocab][D]; the embedding table when the checkpoint ties them
    EncoderW enc;
    int* ids_dev = nullptr;
    long ids_cap = 0;
    int* first_dev = nullptr;  // [max_seqs]
    KvCache cache;             // allocated at the first prefill, kept for the handle's life
    int n_seqs = 0, length = 0;
    int first_host[LM_MAX_SEQS] = {};   // first_dev's values for the n_seqs sequences held (ace355_lm_fan_out plans from them)
    unsigned long long* bad_dev = nullptr;   // out-of-range tokens ace355_lm_decode_tokens replaced; allocated with the cache
    hipStream_t tokens_stream = nullptr;     // the stream of the last ace355_lm_decode_tokens
    char* score_ws = nullptr;                // ace355_lm_score: row list, targets and the rows entry's workspace; grows on demand
    size_t score_cap = 0;
};

namespace {

bool lm_resolve(ace355_lm* h, const std::string& name, PackDest* d) {
    const long D = h->D, V = h->cfg.vocab_size;
    if (name == "lm_head.weight") {
        *d = pack_rows(h->head, 1, V, D, D, 0);
        d->ignore = h->cfg.tie_word_embeddings != 0;   // the same tensor as the embedding table: one copy
        return true;
    }
    if (name.compare(0, 6, "model.") != 0) return false;
    if (name == "model.embed_tokens.weight") { *d = pack_rows(h->embed, 1, V, D, D, 0); return true; }
    if (name == "model.norm.weight") { *d = pack_rows(h->enc.norm, 0, 1, D, D, 0); return true; }
    return resolve_encoder_layers(*h, h->enc, name, 6, d);
}

int lm_check_ids(const ace355_lm* h, const int32_t* ids, long n, const char* who) {
    for (long i = 0; i < n; ++i) {
        if (ids[i] < 0 || ids[i] >= h->cfg.vocab_size) {
            set_error(std::string(who) + ": token id " + std::to_string(ids[i]) + " at position " + std::to_string(i) + " outside [0, " +
                      std::to_string(h->cfg.vocab_size) + ")");
            return ACE355_ERR_INVALID;
        }
    }
    return 0;
}

int lm_refuse(const std::string& msg) {
    set_error(msg);
    return ACE355_ERR_INVALID;
}

int launch_rc() {
    ACE_LAUNCH_CHECK();
    return 0;
}

const char* fan_out_refusal(int why) {   // plan_lm_fan_out's codes
    switch (why) {
        case 1: return "1 .. 16 sequences, before and after";
        case 2: return "src must be non-decreasing";
        case 3: return "src[n] must be in [0, n]";
        default: return "src[n] names a sequence the handle does not hold";
    }
}

// checked host ids -> the handle's device buffer (the caller's array may be reused as soon as this returns)
int lm_upload_ids(ace355_lm* h, const int32_t* ids, long n, hipStream_t s) {
    if (n > h->ids_cap) {
        ACE_HIP(hipStreamSynchronize(s));
        if (h->ids_dev) hipFree(h->ids_dev);
        h->ids_dev = nullptr;
        h->ids_cap = 0;
        const long cap = n > LM_MAX_SEQS ? n : LM_MAX_SEQS;   // a decode step of any fan-out of this prefill fits
        ACE_HIP(hipMalloc((void**)&h->ids_dev, sizeof(int) * cap + 256));
        h->ids_cap = cap;
    }
    ACE_HIP(hipMemcpyAsync(h->ids_dev, ids, sizeof(int) * n, hipMemcpyHostToDevice, s));
    ACE_HIP(hipStreamSynchronize(s));
    return 0;
}

int lm_ensure_cache(ace355_lm* h, hipStream_t s) {
    if (h->cache.kv) return 0;
    KvCache& c = h->cache;
    c.max_seqs = h->cfg.max_seqs;
    c.max_pos = h->cfg.max_positions;
    ALLOC(h->allocs, c.kv, (size_t)h->cfg.num_layers * 2 * c.slab(h->KVH));
    ALLOC(h->allocs, c.part_o, (size_t)c.max_seqs * h->HQ * LM_MAX_SPLITS * 128);
    ALLOC(h->allocs, c.part_ml, (size_t)c.max_seqs * h->HQ * LM_MAX_SPLITS * 2);
    ALLOC(h->allocs, h->first_dev, (size_t)c.max_seqs);
    c.first_dev = h->first_dev;
    ALLOC(h->allocs, h->bad_dev, 1);
    // on the prefill's stream, which the prefill synchronises before it returns: cleared before any stream can count or read
    ACE_HIP(hipMemsetAsync(h->bad_dev, 0, sizeof(unsigned long long), s));
    return 0;
}

// ids[n] = tokens[n % B] for the N <= 16 sequences of a decode step (one wave); a token outside [0, vocab) becomes id 0 and is counted
__global__ __launch_bounds__(64) void lm_tokens_kernel(const int64_t* __restrict__ tokens, int B, int N, int vocab, int* __restrict__ ids,
                                                       unsigned long long* __restrict__ bad) {
    const int n = threadIdx.x;
    if (n >= N) return;
    const int64_t t = tokens[n % B];
    const bool ok = t >= 0 && t < vocab;
    ids[n] = ok ? (int)t : 0;
    if (!ok) atomicAdd(bad, 1ull);
}

// the stack over N x S rows at position pos0 (h->h embedded from ids_dev): the final norm of every row -> xn (bf16 [N * S, D])
int lm_forward(ace355_lm* h, int N, int S, int pos0, hipStream_t s) {
    const EncPassRequest rq = enc_request(*h, h->enc, N, S, false, &h->cache, pos0);
    int rc = ensure_workspace(h, plan_encoder_workspace(&rq, 1, 0, 0), s);
    if (!rc) rc = launch_embed_rows(h->embed, h->ids_dev, h->h, nullptr, (long)N * S, h->D, s);
    if (!rc) rc = run_encoder_pass(h, h->enc, rq, nullptr, h->xn, s, &h->cache);
    return rc;
}

// ... and the head on every sequence's last row
int lm_run(ace355_lm* h, int N, int S, int pos0, float* logits_dev, hipStream_t s) {
    const int rc = lm_forward(h, N, S, pos0, s);
    if (rc) return rc;
    return launch_lm_head(h->xn + (long)(S - 1) * h->D, (long)S * h->D, h->head, logits_dev, N, h->cfg.vocab_size, h->D, s);
}

// the refusals ace355_lm_prefill and ace355_lm_score share, made before anything is launched
int lm_check_prompt(ace355_lm* h, const int32_t* ids_host, const int32_t* first_host, int N, int P, const std::string& who) {
    if (!h->finalized) { set_error(who + ": call ace355_lm_finalize first"); return ACE355_ERR_STATE; }
    ACE_CHECK(N > 0 && P > 0, who + ": sizes");
    if (N > h->cfg.max_seqs)
        return lm_refuse(who + ": " + std::to_string(N) + " sequences, the handle holds max_seqs = " + std::to_string(h->cfg.max_seqs));
    if (P > h->cfg.max_positions)
        return lm_refuse(who + ": " + std::to_string(P) + " positions, the handle holds max_positions = " +
                         std::to_string(h->cfg.max_positions));
    if ((long)N * P > ACE355_LM_MAX_TOKENS)
        return lm_refuse(who + ": N * P = " + std::to_string((long)N * P) + " tokens in one prefill, at most " +
                         std::to_string(ACE355_LM_MAX_TOKENS));
    for (int n = 0; n < N; ++n)
        if (first_host[n] < 0 || first_host[n] >= P)
            return lm_refuse(who + ": first[" + std::to_string(n) + "] = " + std::to_string(first_host[n]) + " outside [0, " +
                             std::to_string(P) + ")");
    return lm_check_ids(h, ids_host, (long)N * P, who.c_str());
}

// ... and what both do once nothing was refused: the previous generation is gone, the cache exists, the ids, `first` and, if any,
// `extra_bytes` of the call's own are on the device, and the stream is synchronised (`first_host` is caller memory)
int lm_begin_prompt(ace355_lm* h, const int32_t* ids_host, const int32_t* first_host, int N, int P, void* extra_dev,
                    const void* extra_host, size_t extra_bytes, hipStream_t s) {
    h->length = 0;
    h->n_seqs = 0;
    int rc = lm_ensure_cache(h, s);
    if (!rc) rc = lm_upload_ids(h, ids_host, (long)N * P, s);
    if (rc) return rc;
    ACE_HIP(hipMemcpyAsync(h->first_dev, first_host, sizeof(int) * N, hipMemcpyHostToDevice, s));
    if (extra_bytes) ACE_HIP(hipMemcpyAsync(extra_dev, extra_host, extra_bytes, hipMemcpyHostToDevice, s));
    ACE_HIP(hipStreamSynchronize(s));
    return 0;
}

// the refusals ace355_lm_decode and ace355_lm_decode_tokens share
int lm_check_step(const ace355_lm* h, const std::string& who) {
    if (h->length <= 0 || h->n_seqs <= 0) return lm_refuse(who + ": no prefill to continue from");
    if (h->length >= h->cfg.max_positions)
        return lm_refuse(who + ": the cache is full (length " + std::to_string(h->length) + " = max_positions)");
    return 0;
}

// ... and their step, once ids_dev holds the step's ids (`rc`: how getting them there went)
int lm_step(ace355_lm* h, int rc, float* logits_dev, hipStream_t s) {
    if (!rc) rc = lm_run(h, h->n_seqs, 1, h->length, logits_dev, s);
    if (rc) { h->length = 0; h->n_seqs = 0; return rc; }   // a failed launch: the cache is not trustworthy
    h->length += 1;
    return ACE355_OK;
}

}  // namespace

extern "C" {

int ace355_lm_create(const ace355_lm_config* cfg, ace355_lm** out) { return ace355_lm_create_ex(cfg, 0, out); }

int ace355_lm_create_ex(const ace355_lm_config* cfg, uint32_t flags, ace355_lm** out) {
    ACE_CHECK(cfg && out, "lm_create: null argument");
    ACE_CHECK((flags & ~(uint32_t)ACE355_LM_ALLOW_GQA4) == 0, "lm_create: unknown flag");
    const bool gqa4 = (flags & ACE355_LM_ALLOW_GQA4) != 0;
    if (cfg->head_dim != 128 || cfg->num_kv_heads <= 0 ||
        !(cfg->num_heads == 2 * cfg->num_kv_heads || (gqa4 && cfg->num_heads == 4 * cfg->num_kv_heads))) {
        set_error(gqa4 ? "lm_create: only head_dim 128 with num_heads == 2 * or 4 * num_kv_heads is supported"
                       : "lm_create: only head_dim 128 with num_heads == 2 * num_kv_heads is supported");
        return ACE355_ERR_UNSUPPORTED;
    }
    ACE_CHECK(cfg->hidden_size > 0 && cfg->hidden_size % 256 == 0 && cfg->intermediate_size > 0 && cfg->intermediate_size % 64 == 0,
              "lm_create: hidden/intermediate size");
    ACE_CHECK(cfg->num_layers >= 0 && cfg->num_layers <= 256 && cfg->vocab_size > 0, "lm_create: layer count / vocabulary");
    ACE_CHECK(cfg->max_seqs >= 1 && cfg->max_seqs <= LM_MAX_SEQS, "lm_create: max_seqs must be 1 .. 16");
    ACE_CHECK(cfg->max_positions >= 1 && cfg->max_positions <= LM_MAX_POSITIONS, "lm_create: max_positions must be 1 .. 16384");
    static_assert(LM_MAX_SEQS == ACE355_LM_MAX_SEQS && LM_MAX_POSITIONS == ACE355_LM_MAX_POSITIONS, "lm_plan.h and ace355.h agree");
    ace355_lm* h = new ace355_lm();
    h->cfg = *cfg;
    enc_init(h, cfg->hidden_size, cfg->intermediate_size, cfg->num_heads, cfg->num_kv_heads, 0, 0, cfg->rms_norm_eps, cfg->rope_theta);
    h->causal = true;
    const bool tied = cfg->tie_word_embeddings != 0;
    int rc = dev_alloc(h->allocs, &h->embed, (size_t)cfg->vocab_size * h->D);
    if (!rc && !tied) rc = dev_alloc(h->allocs, &h->head, (size_t)cfg->vocab_size * h->D);
    if (!rc) rc = alloc_encoder(h, h->enc, cfg->num_layers, 0);
    if (rc) { ace355_lm_destroy(h); return rc; }
    if (tied) h->head = h->embed;
    h->expected_tensors = 2 + (tied ? 0 : 1) + (size_t)cfg->num_layers * 11;
    *out = h;
    return ACE355_OK;
}

void ace355_lm_destroy(ace355_lm* h) {
    if (!h) return;
    hipDeviceSynchronize();
    free_encoder(h);
    if (h->ids_dev) hipFree(h->ids_dev);
    if (h->score_ws) hipFree(h->score_ws);
    delete h;
}

int ace355_lm_load_tensor(ace355_lm* h, const char* name, const void* data, int dtype, int64_t numel, int is_device) {
    ACE_CHECK(h && name && data, "lm_load_tensor: null argument");
    ACE_CHECK(dtype == ACE355_DTYPE_F32 || dtype == ACE355_DTYPE_BF16, "lm_load_tensor: dtype");
    PackDest d;
    if (!lm_resolve(h, name, &d)) return unknown_tensor("lm_load_tensor", name);
    return load_packed(h, d, name, data, dtype, numel, is_device, "lm_load_tensor");
}

int ace355_lm_finalize(ace355_lm* h) {
    ACE_CHECK(h, "lm_finalize: null handle");
    return finalize_loaded(h, "lm_finalize");
}

int ace355_lm_prefill(ace355_lm* h, const int32_t* ids_host, const int32_t* first_host, int N, int P, float* logits_dev, void* stream) {
    ACE_CHECK(h && ids_host && first_host && logits_dev, "lm_prefill: null argument");
    int rc = lm_check_prompt(h, ids_host, first_host, N, P, "lm_prefill");
    if (rc) return rc;
    // nothing was refused: from here on the previous generation is gone
    hipStream_t s = (hipStream_t)stream;
    rc = lm_begin_prompt(h, ids_host, first_host, N, P, nullptr, nullptr, 0, s);
    if (!rc) rc = lm_run(h, N, P, 0, logits_dev, s);
    if (rc) return rc;
    for (int n = 0; n < N; ++n) h->first_host[n] = first_host[n];
    h->n_seqs = N;
    h->length = P;
    return ACE355_OK;
}

int ace355_lm_score(ace355_lm* h, const int32_t* ids_host, const int32_t* first_host, const int32_t* start_host, int N, int P,
                    float* logprob_dev, int32_t* rank_dev, void* stream) {
    ACE_CHECK(h && ids_host && first_host && start_host && logprob_dev && rank_dev, "lm_score: null argument");
    int rc = lm_check_prompt(h, ids_host, first_host, N, P, "lm_score");
    if (rc) return rc;
    long R = 0;
    for (int n = 0; n < N; ++n) {
        if (start_host[n] <= first_host[n] || start_host[n] >= P)
            return lm_refuse("lm_score: start[" + std::to_string(n) + "] = " + std::to_string(start_host[n]) + " outside (first = " +
                             std::to_string(first_host[n]) + ", " + std::to_string(P) + ")");
        R += P - start_host[n];
    }
    hipStream_t s = (hipStream_t)stream;
    const int V = h->cfg.vocab_size, D = (int)h->D;
    // column c of sequence n is predicted by row n * P + c - 1
    std::vector<int32_t> list((size_t)2 * R);
    long r = 0;
    for (int n = 0; n < N; ++n)
        for (int c = start_host[n]; c < P; ++c, ++r) {
            list[r] = n * P + c - 1;
            list[R + r] = ids_host[(long)n * P + c];
        }
    const size_t list_bytes = ((size_t)2 * R * sizeof(int32_t) + 255) & ~(size_t)255;
    const size_t rows_bytes = ace355_lm_score_workspace_bytes((int)R, V);
    ACE_CHECK(rows_bytes > 0, "lm_score: no scoring plan for this handle's vocabulary / hidden size");
    if (list_bytes + rows_bytes > h->score_cap) {
        ACE_HIP(hipStreamSynchronize(s));
        if (h->score_ws) hipFree(h->score_ws);
        h->score_ws = nullptr;
        h->score_cap = 0;
        ACE_HIP(hipMalloc((void**)&h->score_ws, list_bytes + rows_bytes));
        h->score_cap = list_bytes + rows_bytes;
    }
    // nothing was refused: from here on the previous generation is gone, and none follows (`list` is on the device when this returns)
    rc = lm_begin_prompt(h, ids_host, first_host, N, P, h->score_ws, list.data(), (size_t)2 * R * sizeof(int32_t), s);
    if (!rc) rc = lm_forward(h, N, P, 0, s);
    if (rc) return rc;
    const int32_t* rows_dev = (const int32_t*)h->score_ws;
    return ace355_lm_score_rows(h->xn, D, rows_dev, h->head, rows_dev + R, (int)R, V, D, logprob_dev, rank_dev, h->score_ws + list_bytes,
                                rows_bytes, stream);
}

int ace355_lm_fan_out(ace355_lm* h, const int32_t* src_host, int n_new, void* stream) {
    ACE_CHECK(h && src_host, "lm_fan_out: null argument");
    if (h->length <= 0 || h->n_seqs <= 0) return lm_refuse("lm_fan_out: no prefill to fan out");
    if (n_new < 1 || n_new > h->cfg.max_seqs)
        return lm_refuse("lm_fan_out: " + std::to_string(n_new) + " sequences, the handle holds max_seqs = " +
                         std::to_string(h->cfg.max_seqs));
    LmFanOutPlan plan;
    const int why = plan_lm_fan_out(src_host, n_new, h->n_seqs, &plan);
    if (why) return lm_refuse(std::string("lm_fan_out: ") + fan_out_refusal(why) + " (" + std::to_string(h->n_seqs) + " sequences held)");
    ACE_CHECK(h->cache.kv && h->first_dev && h->ids_cap >= n_new, "lm_fan_out: the handle's cache");
    // nothing was refused
    hipStream_t s = (hipStream_t)stream;
    const KvCache& c = h->cache;
    FirstArgs fa{};
    for (int n = 0; n < n_new; ++n) fa.first[n] = h->first_host[src_host[n]];
    int rc = 0;
    for (int w = 0; w < plan.n_waves && !rc; ++w) {
        FanOutArgs a{c.kv, c.slab(h->KVH), (long)h->KVH * c.max_pos * 128, c.max_pos, h->KVH, 2 * h->cfg.num_layers, h->length, 0, {}, {}};
        for (int n = 0; n < n_new; ++n) {
            if (plan.wave_of[n] != w) continue;
            a.dst[a.count] = n;
            a.src[a.count] = src_host[n];
            ++a.count;
        }
        const long total = (long)a.planes * a.Hkv * a.len * 16;
        if (a.count == 0 || total <= 0) continue;   // (a cache without layers)
        hipLaunchKernelGGL(kv_fan_out_kernel, dim3((unsigned)((total + 255) / 256), a.count), dim3(256), 0, s, a);
        rc = launch_rc();
    }
    if (!rc) {
        hipLaunchKernelGGL(lm_set_first_kernel, dim3(1), dim3(64), 0, s, fa, n_new, h->first_dev);
        rc = launch_rc();
    }
    if (rc) { h->length = 0; h->n_seqs = 0; return rc; }   // a failed launch: the cache is not trustworthy
    for (int n = 0; n < n_new; ++n) h->first_host[n] = fa.first[n];
    h->n_seqs = n_new;
    return ACE355_OK;
}

int ace355_lm_fan_out_plan(const int32_t* src, int n_new, int n_old, int32_t* wave_out, int32_t* n_waves_out) {
    ACE_CHECK(src && wave_out && n_waves_out, "lm_fan_out_plan: null argument");
    LmFanOutPlan plan;
    const int why = plan_lm_fan_out(src, n_new, n_old, &plan);
    if (why) return lm_refuse(std::string("lm_fan_out_plan: ") + fan_out_refusal(why));
    for (int n = 0; n < n_new; ++n) wave_out[n] = plan.wave_of[n];
    *n_waves_out = plan.n_waves;
    return ACE355_OK;
}

int ace355_lm_decode(ace355_lm* h, const int32_t* ids_host, float* logits_dev, void* stream) {
    ACE_CHECK(h && ids_host && logits_dev, "lm_decode: null argument");
    int rc = lm_check_step(h, "lm_decode");
    if (!rc) rc = lm_check_ids(h, ids_host, h->n_seqs, "lm_decode");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    return lm_step(h, lm_upload_ids(h, ids_host, h->n_seqs, s), logits_dev, s);
}

int ace355_lm_decode_tokens(ace355_lm* h, const int64_t* tokens_dev, int B, float* logits_dev, void* stream) {
    ACE_CHECK(h && tokens_dev && logits_dev, "lm_decode_tokens: null argument");
    const int refused = lm_check_step(h, "lm_decode_tokens");
    if (refused) return refused;
    if (B < 1 || h->n_seqs % B != 0)
        return lm_refuse("lm_decode_tokens: B = " + std::to_string(B) + " tokens for " + std::to_string(h->n_seqs) +
                         " sequences (n_seqs must be a multiple of B)");
    ACE_CHECK(h->ids_dev && h->ids_cap >= h->n_seqs && h->bad_dev, "lm_decode_tokens: the handle's id buffer");
    static_assert(LM_MAX_SEQS <= 64, "lm_tokens_kernel is one wave");
    hipStream_t s = (hipStream_t)stream;
    h->tokens_stream = s;
    hipLaunchKernelGGL(lm_tokens_kernel, dim3(1), dim3(64), 0, s, tokens_dev, B, h->n_seqs, h->cfg.vocab_size, h->ids_dev, h->bad_dev);
    ACE_LAUNCH_CHECK();   // (nothing of the cache has been touched yet: the handle stays as it was)
    return lm_step(h, 0, logits_dev, s);
}

int64_t ace355_lm_bad_tokens(ace355_lm* h) {
    if (!h) return -1;
    if (!h->bad_dev) return 0;
    unsigned long long n = 0;
    hipStream_t s = h->tokens_stream;
    if (hipMemcpyAsync(&n, h->bad_dev, sizeof(n), hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
    if (hipMemsetAsync(h->bad_dev, 0, sizeof(n), s) != hipSuccess) return -1;
    if (hipStreamSynchronize(s) != hipSuccess) return -1;
    return (int64_t)n;
}

int ace355_lm_length(ace355_lm* h) { return h ? h->length : -1; }

int ace355_lm_decode_plan(int length, int32_t* chunk_out, int32_t* splits_out) {
    ACE_CHECK(length >= 1 && length <= LM_MAX_POSITIONS && chunk_out && splits_out, "lm_decode_plan: length must be 1 .. 16384");
    const LmDecodePlan p = plan_lm_decode(length);
    *chunk_out = p.chunk;
    *splits_out = p.splits;
    return ACE355_OK;
}

}  // extern "C"
