// xattn_probs.hip - cross-attention probabilities for lyric alignment (ace355_dit_cross_attention_maps, ace355_cross_attention_probs).
//
// The reference's lyric timestamps and scores read the probabilities of eager_attention_forward (base.py:352, output_attentions=True):
// P = softmax_fp32(q k^T scale) over the L encoder rows, for a few (layer, query head) pairs.  The flash kernels of attn.hip never hold
// them; this kernel writes them for the requested heads of one layer:
//
//   out[p][n][j][s] = exp(scale q_s . k_j - m_s) / sum_j' exp(scale q_s . k_j' - m_s)     (fp32, j < Skv, s < Sq)
//
// with q = the cross-q GEMM's head-normed bf16 output and k = the condition slot's head-normed bf16 K.  The scores are NOT rounded to
// bf16 before the softmax: the reference's GPU path does that (its matmul runs in bf16), the fp32 oracle does not, and neither does this
// kernel.  The result is then returned in fp32; the handler layout casts it to the caller's dtype (ace355.align.stack).
//
// One workgroup = 64 queries (four 16-column MFMA blocks) of one (sequence, requested head); 4 waves split the key tiles (16 keys each,
// wave w takes tiles w, w + 4, ...).  S^T = K Q^T as in attn3_kernel: keys on the rows of v_mfma_f32_16x16x32_bf16, queries on the
// columns, so a lane's accumulators belong to one query column and an output row out[p][n][j][s0..] is contiguous along s.
//   pass 1: each lane keeps a running (max, sum) per query column over its keys (online rescale); the four lane groups of a column merge
//           through two xor shuffles, the four waves through LDS in wave order 0..3.  The merge is commutative bit for bit, so every lane
//           of every wave holds the same (m, l).
//   pass 2: the scores are recomputed (same MFMA sequence, same bits) and exp2(t - m) / l goes through a per-wave LDS tile to 16-byte
//           stores along s (scalar stores where a row of an odd Sq leaves the 16-byte grid).
// No score buffer, no scratch, no atomics: the bits of a map depend only on its own (q, k) and on Sq / Skv, not on which other heads or
// layers the call requests.  Keys >= Skv and queries >= Sq read clamped rows and are neither counted nor written.  Head dim 128.
#include "common.h"

namespace ace355 {

namespace {

constexpr int XQ = 64;        // queries per workgroup
constexpr int XK = 16;        // keys per tile (MFMA rows)
constexpr int XW = 4;         // waves
constexpr int XP = XQ + 4;    // LDS row pitch of the staged output tile (floats)

__global__ __launch_bounds__(XW * 64) void xattn_probs_kernel(XattnArgs a, float scale_log2) {
    __shared__ __attribute__((aligned(16))) float sP[XW][XK][XP];
    __shared__ float sM[XW][XQ], sL[XW][XQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = blockIdx.x * XQ, p = blockIdx.y, n = blockIdx.z;
    const int h = a.heads[p], hkv = h / (a.Hq / a.Hkv);
    const int col = lane & 15, grp = lane >> 4;   // MFMA column / row group of this lane

    // Q fragments (B operand): query q0 + 16 cb + col, d = 32 ks + 8 grp .. + 8
    bf16x8 qf[4][4];
    const bf16_t* qb = a.q + (long)n * a.q_seq_stride + h * 128 + 8 * grp;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
        const int s = min(q0 + 16 * cb + col, a.Sq - 1);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[cb][ks] = as_bf16x8(ldg16(qb + (long)s * a.q_ld + 32 * ks));
    }
    const bf16_t* kb = reinterpret_cast<const bf16_t*>(a.k_tab[n]) + hkv * 128 + 8 * grp;
    const int ntiles = (a.Skv + XK - 1) / XK;

    // scores t = scale log2(e) (k . q) of tile kt: acc[cb][i] = key kt XK + 4 grp + i, query q0 + 16 cb + col
    auto scores = [&](int kt, f32x4 (&acc)[4]) {
        bf16x8 kf[4];
        const int j = min(kt * XK + col, a.Skv - 1);   // A operand: key row kt XK + col
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) kf[ks] = as_bf16x8(ldg16(kb + (long)j * a.k_ld + 32 * ks));
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[ks], qf[cb][ks], acc[cb], 0, 0, 0);
        }
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[cb][i] = kt * XK + 4 * grp + i < a.Skv ? acc[cb][i] * scale_log2 : -INFINITY;
    };

    // ---- pass 1: (max, sum) per query column
    float m[4], l[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) m[cb] = -1e30f, l[cb] = 0.f;   // (finite start: a lane whose keys are all masked keeps l = 0)
    for (int kt = wave; kt < ntiles; kt += XW) {
        f32x4 acc[4];
        scores(kt, acc);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const float mx = fmaxf(m[cb], fmaxf(fmaxf(acc[cb][0], acc[cb][1]), fmaxf(acc[cb][2], acc[cb][3])));
            float e = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) e += exp2f(acc[cb][i] - mx);
            l[cb] = l[cb] * exp2f(m[cb] - mx) + e;
            m[cb] = mx;
        }
    }
    auto merge = [](float& m1, float& l1, float m2, float l2) {   // commutative bit for bit
        const float mx = fmaxf(m1, m2);
        l1 = l1 * exp2f(m1 - mx) + l2 * exp2f(m2 - mx);
        m1 = mx;
    };
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float m2 = __shfl_xor(m[cb], o, 64), l2 = __shfl_xor(l[cb], o, 64);
            merge(m[cb], l[cb], m2, l2);
        }
        if (grp == 0) sM[wave][16 * cb + col] = m[cb], sL[wave][16 * cb + col] = l[cb];
    }
    __syncthreads();
    float inv[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
        float mm = sM[0][16 * cb + col], ll = sL[0][16 * cb + col];
        for (int w = 1; w < XW; ++w) merge(mm, ll, sM[w][16 * cb + col], sL[w][16 * cb + col]);
        m[cb] = mm;
        inv[cb] = 1.0f / ll;
    }

    // ---- pass 2: probabilities, staged per wave for stores along s.  Every wave runs the same trip count (barriers); a wave past the
    //      last tile only takes part in them.
    float* ob = a.out + ((long)p * a.N + n) * a.Skv * a.Sq;
    const int iters = (ntiles + XW - 1) / XW;
    for (int it = 0; it < iters; ++it) {
        const int kt = wave + XW * it;
        if (kt < ntiles) {
            f32x4 acc[4];
            scores(kt, acc);
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int i = 0; i < 4; ++i) sP[wave][4 * grp + i][16 * cb + col] = exp2f(acc[cb][i] - m[cb]) * inv[cb];
        }
        __syncthreads();
        if (kt < ntiles) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {   // 16 rows x 16 float4 per wave tile
                const int e = lane + 64 * r, row = e >> 4, c = (e & 15) * 4;
                const int j = kt * XK + row, s = q0 + c;
                if (j >= a.Skv || s >= a.Sq) continue;
                float* dst = ob + (long)j * a.Sq + s;
                const float4 v = *reinterpret_cast<const float4*>(&sP[wave][row][c]);
                if (s + 4 <= a.Sq && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
                    *reinterpret_cast<float4*>(dst) = v;
                } else {
                    dst[0] = v.x;
                    if (s + 1 < a.Sq) dst[1] = v.y;
                    if (s + 2 < a.Sq) dst[2] = v.z;
                    if (s + 3 < a.Sq) dst[3] = v.w;
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace

int launch_xattn_probs(const XattnArgs& a, hipStream_t s) {
    ACE_CHECK(a.q && a.out && a.N > 0 && a.N <= 64 && a.Sq > 0 && a.Skv > 0, "xattn_probs: empty problem");
    ACE_CHECK(a.Hkv > 0 && a.Hq % a.Hkv == 0 && a.n_heads > 0 && a.n_heads <= XATTN_MAX_HEADS, "xattn_probs: heads");
    ACE_CHECK(a.q_ld % 8 == 0 && a.k_ld % 8 == 0 && a.q_ld >= a.Hq * 128 && a.k_ld >= a.Hkv * 128 && a.q_seq_stride % 8 == 0,
              "xattn_probs: leading dimensions must be multiples of 8 and hold every head");
    ACE_CHECK((reinterpret_cast<uintptr_t>(a.q) & 15) == 0, "xattn_probs: q must be 16-byte aligned");
    for (int i = 0; i < a.N; ++i) ACE_CHECK(a.k_tab[i] && (a.k_tab[i] & 15) == 0, "xattn_probs: k must be 16-byte aligned");
    for (int p = 0; p < a.n_heads; ++p) ACE_CHECK(a.heads[p] >= 0 && a.heads[p] < a.Hq, "xattn_probs: head out of range");
    const float scale_log2 = a.scale * 1.4426950408889634f;
    hipLaunchKernelGGL(xattn_probs_kernel, dim3((a.Sq + XQ - 1) / XQ, a.n_heads, a.N), dim3(XW * 64), 0, s, a, scale_log2);
    ACE_LAUNCH_CHECK();
    return 0;
}

}  // namespace ace355
