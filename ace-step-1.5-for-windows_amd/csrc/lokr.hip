// lokr.hip - LoKr (LyCORIS Kronecker) adapters merged into the packed DiT weights (ace355_dit_set_adapters_mixed).  One term on a
// target [out, in] = [out_l out_k, in_m in_n]:  dW[l out_k + k, m in_n + n] = scale W1[l, m] W2[k, n], W1 / W2 given in full or as a
// low-rank product.  The merge writes bf16_rne(float(W0) + sum_j dW_j) over the packed rows, exactly as the LoRA merge (lora.hip)
// does: fp32 products and sums, the terms in call order, one rounding.  A pure stream over the weights: the arithmetic per element is
// two LDS reads and one multiply-add.
#include "../../include/ace355.h"
#include "common.h"
#include "dora.h"

namespace ace355 {

namespace {

constexpr int TM = LOKR_TILE_ROWS;   // source rows of a tile
constexpr int TN = LOKR_TILE_COLS;   // columns of a tile
constexpr int FM = LOKR_FACTOR_ROWS, FN = LOKR_FACTOR_COLS;   // factor pre-pass tile
constexpr int KC = 32;               // rank step = the K of one v_mfma_f32_16x16x32_bf16
constexpr int KP = KC + 8;           // LDS row pitch of the staged operands (80 bytes: 16-byte fragment reads stay aligned)

// Factor pre-pass.  One workgroup = one (factor, FM rows, FN columns) tile of dst = a @ b; 4 waves, wave w owns rows [16w, 16w + 16).
// a rows and b columns are staged 32 ranks at a time, zero beyond the rank and beyond the factor's edges (any rank >= 1 works), and
// accumulated in fp32 in rank order, as lora_merge_kernel does for B.A.
__global__ __launch_bounds__(256) void lokr_factor_kernel(const KronFactorDev* __restrict__ jobs, int n_jobs) {
    __shared__ __attribute__((aligned(16))) bf16_t sA[FM][KP];
    __shared__ __attribute__((aligned(16))) bf16_t sBt[FN][KP];
    const int bid = blockIdx.x;
    int lo = 0, hi = n_jobs - 1;   // last job whose first tile is <= bid (jobs are in tile order)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].tile0 <= bid) lo = mid;
        else hi = mid - 1;
    }
    const KronFactorDev f = jobs[lo];
    const int local = bid - f.tile0;
    const int n0 = (local / f.tiles_n) * FM, c0 = (local % f.tiles_n) * FN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    f32x4 acc[FN / 16];
    for (int b = 0; b < FN / 16; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < f.rank; k0 += KC) {
        for (int e = tid; e < FM * KC; e += 256) {   // a [rows, rank]: rows n0.., ranks k0..
            const int r = e / KC, k = e % KC, n = n0 + r, kk = k0 + k;
            sA[r][k] = (n < f.rows && kk < f.rank) ? f.a[(long)n * f.rank + kk] : (bf16_t)0;
        }
        for (int e = tid; e < KC * FN; e += 256) {   // b [rank, cols]: ranks k0.., columns c0.. -> transposed, rank-contiguous
            const int k = e / FN, c = e % FN, kk = k0 + k, cc = c0 + c;
            sBt[c][k] = (kk < f.rank && cc < f.cols) ? f.b[(long)kk * f.cols + cc] : (bf16_t)0;
        }
        __syncthreads();
        // lane l: A operand = a[row l & 15][k 8(l >> 4) + i], B operand = b[k 8(l >> 4) + i][column l & 15]
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(&sA[wave * 16 + (lane & 15)][8 * (lane >> 4)]);
        for (int b = 0; b < FN / 16; ++b) {
            const bf16x8 x = *reinterpret_cast<const bf16x8*>(&sBt[b * 16 + (lane & 15)][8 * (lane >> 4)]);
            acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, x, acc[b], 0, 0, 0);
        }
        __syncthreads();
    }
    for (int b = 0; b < FN / 16; ++b)   // C / D of the 16x16 tile: column l & 15, rows 4(l >> 4) + i
        for (int i = 0; i < 4; ++i) {
            const int n = n0 + wave * 16 + (lane >> 4) * 4 + i, c = c0 + b * 16 + (lane & 15);
            if (n < f.rows && c < f.cols) f.dst[(long)n * f.cols + c] = acc[b][i];
        }
}

__device__ __forceinline__ float factor_at(const void* p, int is_f32, long i) {
    return is_f32 ? reinterpret_cast<const float*>(p)[i] : bf2f(reinterpret_cast<const bf16_t*>(p)[i]);
}

// Merge.  One workgroup = one (target, TM source rows, TN columns) tile; a thread owns 4 groups of 8 columns (rows r, r + 16, ...),
// whose pristine 16 bytes it loads first.  Per term the tile's sub-blocks go to LDS in fp32: s1 = scale x W1[l0 .. l0 + nl)[m0 .. m0 + nm)
// and s2 = W2 rows x columns, indexed by k / n themselves while W2 fits the tile (out_k <= TM resp. in_n <= TN) and by the tile's own
// row / column otherwise (W2 larger than a tile: k = (n0 + r) mod out_k wraps at most once).  Every read is inside its factor.
// A term with in_n % 8 == 0, in_n <= TN and a 16-byte aligned W2 (KronTermDev::wide) takes 16-byte paths: an 8-column group then lies
// inside one m, W2 is staged 8 columns per load and read back as two float4.  Both paths form the same fp32 values.
// PASS 0 is that merge.  PASS 1 / 2 are the two passes of a DoRA target (dora.h): the same fp32 values, reduced resp. rescaled.
template <int PASS>
__global__ __launch_bounds__(256) void lokr_merge_kernel(const LoraTargetDev* __restrict__ tg, int n_targets,
                                                         const KronTermDev* __restrict__ terms, const DoraDev* __restrict__ dora) {
    extern __shared__ __attribute__((aligned(16))) float pool[];
    const int bid = blockIdx.x;
    int lo = 0, hi = n_targets - 1;   // last target whose first tile is <= bid (targets are in tile order)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tg[mid].tile0 <= bid) lo = mid;
        else hi = mid - 1;
    }
    const LoraTargetDev t = tg[lo];
    const int local = bid - t.tile0;
    const int n0 = (local / t.tiles_n) * TM, c0 = (local % t.tiles_n) * TN;
    const int tid = threadIdx.x;
    const int c8 = (tid & 15) * 8, rb = tid >> 4;   // this thread's column group and its first row; rows rb + 16 i

    constexpr int G = TM / 16;
    uint4 w[G];
    long off[G];
    bool live[G];
#pragma unroll
    for (int i = 0; i < G; ++i) {
        const int n = n0 + rb + 16 * i, c = c0 + c8;
        live[i] = n < t.rows && c < t.cols;   // (cols % 8 == 0: a group is inside or outside as a whole)
        off[i] = live[i] ? pack_row(t.mode, n, t.row0, t.p0) * t.ld + c : 0;
        w[i] = live[i] ? *reinterpret_cast<const uint4*>(t.src + off[i]) : uint4{0u, 0u, 0u, 0u};
    }
    float sum[G][8];
#pragma unroll
    for (int i = 0; i < G; ++i)
#pragma unroll
        for (int q = 0; q < 8; ++q) sum[i][q] = 0.f;

    const int rlast = min(n0 + TM, t.rows) - 1, clast = min(c0 + TN, t.cols) - 1;
    const int col = min(c0 + c8, clast);   // (a thread without a live group still indexes inside the staged blocks)
    for (int j = 0; j < t.nterms; ++j) {
        const KronTermDev u = terms[t.term0 + j];
        const int l0 = n0 / u.out_k, nl = rlast / u.out_k - l0 + 1;
        const int m0 = c0 / u.in_n, nm = clast / u.in_n - m0 + 1;
        const bool byk = u.out_k <= TM, byn = u.in_n <= TN;
        const int nk = byk ? u.out_k : TM, nn = byn ? u.in_n : TN, p2 = lokr_w2_pitch(nn);
        const int kb = n0 - l0 * u.out_k, nb = c0 - m0 * u.in_n;   // k / n of the tile's first row / column
        float* s1 = pool;
        float* s2 = pool + ((nl * nm + 3) & ~3);
        for (int li = tid >> 6; li < nl; li += 4)
            for (int mi = tid & 63; mi < nm; mi += 64)
                s1[li * nm + mi] = u.scale * factor_at(u.w1, u.w1_f32, (long)(l0 + li) * u.in_m + m0 + mi);
        if (u.wide) {
            const int nv = nn >> 3;   // 8-column vectors per W2 row
            for (int e = tid; e < nk * nv; e += 256) {
                const int ri = e / nv, ci = (e - ri * nv) * 8;
                int k = ri;
                if (!byk) { k += kb; if (k >= u.out_k) k -= u.out_k; }
                const long at = (long)k * u.in_n + ci;
                float4 lo4, hi4;
                if (u.w2_f32) {
                    lo4 = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(u.w2) + at);
                    hi4 = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(u.w2) + at + 4);
                } else {
                    const uint4 v = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(u.w2) + at);
                    lo4 = float4{bf_lo(v.x), bf_hi(v.x), bf_lo(v.y), bf_hi(v.y)};
                    hi4 = float4{bf_lo(v.z), bf_hi(v.z), bf_lo(v.w), bf_hi(v.w)};
                }
                *reinterpret_cast<float4*>(&s2[ri * p2 + ci]) = lo4;
                *reinterpret_cast<float4*>(&s2[ri * p2 + ci + 4]) = hi4;
            }
        } else {
            for (int ri = tid >> 6; ri < nk; ri += 4) {
                int k = ri;
                if (!byk) { k += kb; if (k >= u.out_k) k -= u.out_k; }
                for (int ci = tid & 63; ci < nn; ci += 64) {
                    int n = ci;
                    if (!byn) { n += nb; if (n >= u.in_n) n -= u.in_n; }
                    s2[ri * p2 + ci] = factor_at(u.w2, u.w2_f32, (long)k * u.in_n + n);
                }
            }
        }
        __syncthreads();
        const int mc = col / u.in_n, nc = col - mc * u.in_n;   // m, n of this thread's first column
#pragma unroll
        for (int i = 0; i < G; ++i) {
            if (!live[i]) continue;
            const int r = rb + 16 * i, row = n0 + r, l = row / u.out_k, k = row - l * u.out_k;
            const float* a = s1 + (l - l0) * nm + (mc - m0);
            const float* b = s2 + (byk ? k : r) * p2;
            if (u.wide) {
                const float a0 = a[0];
                const float4 b0 = *reinterpret_cast<const float4*>(b + nc), b1 = *reinterpret_cast<const float4*>(b + nc + 4);
                sum[i][0] += a0 * b0.x; sum[i][1] += a0 * b0.y; sum[i][2] += a0 * b0.z; sum[i][3] += a0 * b0.w;
                sum[i][4] += a0 * b1.x; sum[i][5] += a0 * b1.y; sum[i][6] += a0 * b1.z; sum[i][7] += a0 * b1.w;
            } else {
                int m = 0, n = nc;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    sum[i][q] += a[m] * b[byn ? n : c8 + q];
                    if (++n == u.in_n) { n = 0; ++m; }
                }
            }
        }
        __syncthreads();
    }
    if constexpr (PASS != 0) {
        __shared__ double sQ[DORA_LDS_DOUBLES];
        float v[G][8];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            v[i][0] = bf_lo(w[i].x) + sum[i][0]; v[i][1] = bf_hi(w[i].x) + sum[i][1];
            v[i][2] = bf_lo(w[i].y) + sum[i][2]; v[i][3] = bf_hi(w[i].y) + sum[i][3];
            v[i][4] = bf_lo(w[i].z) + sum[i][4]; v[i][5] = bf_hi(w[i].z) + sum[i][5];
            v[i][6] = bf_lo(w[i].w) + sum[i][6]; v[i][7] = bf_hi(w[i].w) + sum[i][7];
        }
        dora_epilogue<PASS>(t, dora[lo], n0, c0, tid, v, live, off, sQ);
        return;
    }
#pragma unroll
    for (int i = 0; i < G; ++i) {
        if (!live[i]) continue;
        uint4 o = w[i];   // no term (a target restored to its base): the pristine bits, signed zeros included
        if (t.nterms) {
            o.x = pack_bf2(bf_lo(w[i].x) + sum[i][0], bf_hi(w[i].x) + sum[i][1]);
            o.y = pack_bf2(bf_lo(w[i].y) + sum[i][2], bf_hi(w[i].y) + sum[i][3]);
            o.z = pack_bf2(bf_lo(w[i].z) + sum[i][4], bf_hi(w[i].z) + sum[i][5]);
            o.w = pack_bf2(bf_lo(w[i].w) + sum[i][6], bf_hi(w[i].w) + sum[i][7]);
        }
        *reinterpret_cast<uint4*>(t.dst + off[i]) = o;
    }
}

}  // namespace

int launch_lokr_factors(const KronFactorDev* jobs_dev, int n_jobs, int total_tiles, hipStream_t s) {
    if (n_jobs <= 0 || total_tiles <= 0) return 0;
    hipLaunchKernelGGL(lokr_factor_kernel, dim3(total_tiles), dim3(256), 0, s, jobs_dev, n_jobs);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_lokr_merge(const LoraTargetDev* targets_dev, int n_targets, int total_tiles, const KronTermDev* terms_dev, int lds_floats,
                      hipStream_t s, const DoraDev* dora_dev, int pass) {
    if (n_targets <= 0 || total_tiles <= 0) return 0;
    if (lds_floats < 4 || lds_floats > LOKR_LDS_FLOATS) { set_error("lokr merge: LDS size out of range"); return ACE355_ERR_INVALID; }
    if (pass < 0 || pass > 2 || (pass != 0 && !dora_dev)) { set_error("lokr merge: pass"); return ACE355_ERR_INVALID; }
    auto* k = pass == 0 ? lokr_merge_kernel<0> : pass == 1 ? lokr_merge_kernel<1> : lokr_merge_kernel<2>;
    hipLaunchKernelGGL(k, dim3(total_tiles), dim3(256), (size_t)lds_floats * sizeof(float), s, targets_dev, n_targets, terms_dev,
                       dora_dev);
    ACE_LAUNCH_CHECK();
    return 0;
}

}  // namespace ace355
