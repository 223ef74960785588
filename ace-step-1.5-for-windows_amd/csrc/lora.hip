// lora.hip - LoRA adapters merged into the packed DiT weights (ace355_dit_set_adapters) and the read-back of a packed weight in the
// reference layout (ace355_dit_read_weight).  PEFT's unmerged eval forward y = x W^T + s (x A^T) B^T equals a forward with W + s B A;
// the merge writes bf16_rne(float(W0) + sum_j s_j B_j A_j) over the packed rows the GEMM / attention kernels already read, so those
// kernels and every result without an adapter stay as they are.
#include "../../include/ace355.h"
#include "common.h"
#include "dora.h"

namespace ace355 {

namespace {

constexpr int TM = LORA_TILE_ROWS;   // source rows of a tile
constexpr int TN = LORA_TILE_COLS;   // columns of a tile
constexpr int KC = 32;               // rank step = the K of one v_mfma_f32_16x16x32_bf16
constexpr int KP = KC + 8;           // LDS row pitch of the staged operands (80 bytes: 16-byte fragment reads stay aligned)
constexpr int SP = TN + 4;           // LDS row pitch of the fp32 sum tile

// One workgroup = one (target, TM source rows, TN columns) tile; 4 waves, wave w owns rows [16w, 16w + 16) x all TN columns as
// TN / 16 accumulators of 16 x 16.  Per term: B rows and A columns staged in LDS 32 ranks at a time (zero beyond the rank: any rank
// works), B.A into the term's own fp32 accumulators, then sum += scale x acc in fp32.  Epilogue: the sum tile goes through LDS so
// that the pristine read and the live write are 16-byte accesses along a packed row, at the row the pack row map gives.
// PASS 0 is that merge.  PASS 1 / 2 are the two passes of a DoRA target (dora.h): the same fp32 values, reduced resp. rescaled.
template <int PASS>
__global__ __launch_bounds__(256) void lora_merge_kernel(const LoraTargetDev* __restrict__ tg, int n_targets,
                                                         const LoraTermDev* __restrict__ terms, const DoraDev* __restrict__ dora) {
    __shared__ __attribute__((aligned(16))) bf16_t sB[TM][KP];
    __shared__ __attribute__((aligned(16))) bf16_t sAt[TN][KP];
    __shared__ __attribute__((aligned(16))) float sS[TM][SP];
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
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    f32x4 sum[TN / 16];
    for (int b = 0; b < TN / 16; ++b) sum[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < t.nterms; ++j) {
        const LoraTermDev u = terms[t.term0 + j];
        f32x4 acc[TN / 16];
        for (int b = 0; b < TN / 16; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < u.rank; k0 += KC) {
            for (int e = tid; e < TM * KC; e += 256) {   // B [out, rank]: rows n0.., ranks k0..
                const int r = e / KC, k = e % KC, n = n0 + r, kk = k0 + k;
                sB[r][k] = (n < t.rows && kk < u.rank) ? u.B[(long)n * u.rank + kk] : (bf16_t)0;
            }
            for (int e = tid; e < KC * TN; e += 256) {   // A [rank, in]: ranks k0.., columns c0.. -> transposed, rank-contiguous
                const int k = e / TN, c = e % TN, kk = k0 + k, cc = c0 + c;
                sAt[c][k] = (kk < u.rank && cc < t.cols) ? u.A[(long)kk * t.cols + cc] : (bf16_t)0;
            }
            __syncthreads();
            // lane l: A operand = B[row l & 15][k 8(l >> 4) + i], B operand = A[k 8(l >> 4) + i][column l & 15]
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(&sB[wave * 16 + (lane & 15)][8 * (lane >> 4)]);
            for (int b = 0; b < TN / 16; ++b) {
                const bf16x8 x = *reinterpret_cast<const bf16x8*>(&sAt[b * 16 + (lane & 15)][8 * (lane >> 4)]);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, x, acc[b], 0, 0, 0);
            }
            __syncthreads();
        }
        for (int b = 0; b < TN / 16; ++b) sum[b] += u.scale * acc[b];
    }
    if (t.nterms) {   // C / D of the 16x16 tile: column l & 15, rows 4(l >> 4) + i
        for (int b = 0; b < TN / 16; ++b)
            for (int i = 0; i < 4; ++i) sS[wave * 16 + (lane >> 4) * 4 + i][b * 16 + (lane & 15)] = sum[b][i];
        __syncthreads();
    }
    if constexpr (PASS != 0) {
        __shared__ double sQ[DORA_LDS_DOUBLES];
        float v[4][8];
        long off[4];
        bool live[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {   // (the groups the loop below gives this thread)
            const int r = (tid >> 4) + 16 * i, c8 = (tid & 15) * 8, n = n0 + r, c = c0 + c8;
            live[i] = n < t.rows && c < t.cols;
            off[i] = live[i] ? pack_row(t.mode, n, t.row0, t.p0) * t.ld + c : 0;
            const uint4 w = live[i] ? *reinterpret_cast<const uint4*>(t.src + off[i]) : uint4{0u, 0u, 0u, 0u};
            float4 s0 = float4{0.f, 0.f, 0.f, 0.f}, s1 = s0;
            if (t.nterms) {
                s0 = *reinterpret_cast<const float4*>(&sS[r][c8]);
                s1 = *reinterpret_cast<const float4*>(&sS[r][c8 + 4]);
            }
            v[i][0] = bf_lo(w.x) + s0.x; v[i][1] = bf_hi(w.x) + s0.y; v[i][2] = bf_lo(w.y) + s0.z; v[i][3] = bf_hi(w.y) + s0.w;
            v[i][4] = bf_lo(w.z) + s1.x; v[i][5] = bf_hi(w.z) + s1.y; v[i][6] = bf_lo(w.w) + s1.z; v[i][7] = bf_hi(w.w) + s1.w;
        }
        dora_epilogue<PASS>(t, dora[lo], n0, c0, tid, v, live, off, sQ);
        return;
    }
    for (int e = tid; e < TM * TN / 8; e += 256) {
        const int r = e / (TN / 8), c8 = (e % (TN / 8)) * 8, n = n0 + r, c = c0 + c8;
        if (n >= t.rows || c >= t.cols) continue;
        const long off = pack_row(t.mode, n, t.row0, t.p0) * t.ld + c;
        const uint4 w = *reinterpret_cast<const uint4*>(t.src + off);
        uint4 o = w;   // no term (a target restored to its base): the pristine bits, signed zeros included
        if (t.nterms) {
            const float4 s0 = *reinterpret_cast<const float4*>(&sS[r][c8]);
            const float4 s1 = *reinterpret_cast<const float4*>(&sS[r][c8 + 4]);
            o.x = pack_bf2(bf_lo(w.x) + s0.x, bf_hi(w.x) + s0.y);
            o.y = pack_bf2(bf_lo(w.y) + s0.z, bf_hi(w.y) + s0.w);
            o.z = pack_bf2(bf_lo(w.z) + s1.x, bf_hi(w.z) + s1.y);
            o.w = pack_bf2(bf_lo(w.w) + s1.z, bf_hi(w.w) + s1.w);
        }
        *reinterpret_cast<uint4*>(t.dst + off) = o;
    }
}

__global__ void lora_read_kernel(const bf16_t* __restrict__ w, long ld, int mode, long row0, int p0, long rows, long cols,
                                 void* __restrict__ dst, int dst_is_bf16) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cols) return;
    const long r = i / cols, c = i - r * cols;
    const bf16_t v = w[pack_row(mode, r, row0, p0) * ld + c];
    if (dst_is_bf16) reinterpret_cast<bf16_t*>(dst)[i] = v;
    else reinterpret_cast<float*>(dst)[i] = bf2f(v);
}

}  // namespace

int launch_lora_merge(const LoraTargetDev* targets_dev, int n_targets, int total_tiles, const LoraTermDev* terms_dev, hipStream_t s,
                      const DoraDev* dora_dev, int pass) {
    if (n_targets <= 0 || total_tiles <= 0) return 0;
    if (pass < 0 || pass > 2 || (pass != 0 && !dora_dev)) { set_error("lora merge: pass"); return ACE355_ERR_INVALID; }
    auto* k = pass == 0 ? lora_merge_kernel<0> : pass == 1 ? lora_merge_kernel<1> : lora_merge_kernel<2>;
    hipLaunchKernelGGL(k, dim3(total_tiles), dim3(256), 0, s, targets_dev, n_targets, terms_dev, dora_dev);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_lora_read(const bf16_t* w, long ld, int mode, long row0, int p0, long rows, long cols, void* dst, int dst_is_bf16,
                     hipStream_t s) {
    const long n = rows * cols;
    hipLaunchKernelGGL(lora_read_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, ld, mode, row0, p0, rows, cols, dst,
                       dst_is_bf16);
    ACE_LAUNCH_CHECK();
    return 0;
}

}  // namespace ace355
