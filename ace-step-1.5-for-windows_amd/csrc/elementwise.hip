// elementwise.hip - HBM-bound kernels of the DiT path: RMSNorm+modulation, head-RMSNorm+RoPE, V transpose,
// timestep-embedding GEMVs, patchify input packing, the APG + Euler sampler step, weight packing, post-processing.
// All are wave64 kernels with 8/16-byte vector accesses and shuffle reductions (no LDS unless transposing).
#include "common.h"

#include <math.h>

#include <vector>

namespace ace355 {

namespace {

// ------------------------------------------------------------------------------------------------
// y = bf16( w * (x * rsqrt(mean(x^2) + eps)) * (1 + sc) + sh )     (Qwen3RMSNorm + base.py:499,530,1496)
// one wave per row; x f32 [M, D]
template <int NCH>  // NCH = D / 256 float4 chunks per lane held in registers (0: generic two-pass)
__global__ __launch_bounds__(256) void rmsnorm_mod_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          bf16_t* __restrict__ y, int M, int D, float eps,
                                                          const float* __restrict__ sc1, const float* __restrict__ sc2,
                                                          const float* __restrict__ sh1, const float* __restrict__ sh2,
                                                          int stride, int rows_per_seq) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= M) return;
    const float* xr = x + (long)row * D;
    float4 xv[NCH > 0 ? NCH : 1];
    float ss = 0.f;
    if (NCH > 0) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            xv[i] = *reinterpret_cast<const float4*>(xr + i * 256 + lane * 4);
            ss += xv[i].x * xv[i].x + xv[i].y * xv[i].y + xv[i].z * xv[i].z + xv[i].w * xv[i].w;
        }
    } else {
        for (int c = lane * 4; c < D; c += 256) {
            const float4 v = *reinterpret_cast<const float4*>(xr + c);
            ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
    }
    ss = wave_sum(ss);
    const float rstd = rsqrtf(ss / (float)D + eps);
    const long so = sc1 ? (long)(row / rows_per_seq) * stride : 0;
    bf16_t* yr = y + (long)row * D;
    auto emit = [&](int c, const float4 v) {
        const float4 ww = *reinterpret_cast<const float4*>(w + c);
        float o0 = ww.x * (v.x * rstd), o1 = ww.y * (v.y * rstd), o2 = ww.z * (v.z * rstd), o3 = ww.w * (v.w * rstd);
        if (sc1) {
            const float4 a = *reinterpret_cast<const float4*>(sc1 + c);
            const float4 b = *reinterpret_cast<const float4*>(sc2 + so + c);
            const float4 e = *reinterpret_cast<const float4*>(sh1 + c);
            const float4 f = *reinterpret_cast<const float4*>(sh2 + so + c);
            o0 = o0 * (1.f + (a.x + b.x)) + (e.x + f.x);
            o1 = o1 * (1.f + (a.y + b.y)) + (e.y + f.y);
            o2 = o2 * (1.f + (a.z + b.z)) + (e.z + f.z);
            o3 = o3 * (1.f + (a.w + b.w)) + (e.w + f.w);
        }
        *reinterpret_cast<uint2*>(yr + c) = make_uint2(pack_bf2(o0, o1), pack_bf2(o2, o3));
    };
    if (NCH > 0) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) emit(i * 256 + lane * 4, xv[i]);
    } else {
        for (int c = lane * 4; c < D; c += 256) emit(c, *reinterpret_cast<const float4*>(xr + c));
    }
}

// ------------------------------------------------------------------------------------------------
// The same norm with the per-column factors folded beforehand: y = bf16( (x * rstd) * g + sft ), g = w * (1 + sc1 + sc2),
// sft = sh1 + sh2.  The five-vector form above reads 40 KB of (cached) vectors per 8 KB row and was bound by those loads
// (19.4 us at M = 6000 against 14.1 us unmodulated); the DiT folds the vectors of all layers once per forward
// (mod_gs_kernel) and streams x through this kernel: 8 consecutive columns per lane, one 16-byte store per 8 outputs.
// MXQ: the output leaves as OCP MXFP8 (the operand of an MX GEMM) instead of bf16: q fp8 e4m3 [M, D] at `y`, E8M0 block scales at
// `mxs` ([D / 128][mx_pad] words, GemmEpilogue::mx_sa layout).  The value that is quantised is the BF16-ROUNDED norm output, so the
// fused kernel is bit-identical to rmsnorm -> mx_quant_kernel.  A 32-column block = 4 neighbouring lanes of a pass, a scale word = 16.
__device__ __forceinline__ int mx_block_exp(float amax) {
    int sb = (int)((__float_as_uint(amax) >> 23) & 0xffu) - 8;
    return sb < 0 ? 0 : (sb > 254 ? 254 : sb);
}
__device__ __forceinline__ uint32_t mx_pack4(float a0, float a1, float a2, float a3, float inv) {
    a0 = fminf(fmaxf(a0 * inv, -448.f), 448.f); a1 = fminf(fmaxf(a1 * inv, -448.f), 448.f);
    a2 = fminf(fmaxf(a2 * inv, -448.f), 448.f); a3 = fminf(fmaxf(a3 * inv, -448.f), 448.f);
    int pk = __builtin_amdgcn_cvt_pk_fp8_f32(a0, a1, 0, false);
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a2, a3, pk, true);
}
template <int NP, bool SHIFT, bool MXQ = false>  // NP = D / 512 passes held in registers (0: generic two-pass); SHIFT: sft != nullptr
__global__ __launch_bounds__(256) void rmsnorm_gs_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                         const float* __restrict__ sft, bf16_t* __restrict__ y, int M, int D,
                                                         float eps, long stride, int rows_per_seq, uint32_t* __restrict__ mxs = nullptr,
                                                         int mx_pad = 0) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= M) return;
    const float* xr = x + (long)row * D;
    const long so = stride ? (long)(row / rows_per_seq) * stride : 0;
    const float* gp = g + so;
    const float* sp = SHIFT ? sft + so : nullptr;
    bf16_t* yr = y + (long)row * D;
    auto emit = [&](int c, const f32x4 a, const f32x4 b, const f32x4 ga, const f32x4 gb, const f32x4 sa, const f32x4 sb, float rstd) {
        float o[8] = {(a[0] * rstd) * ga[0], (a[1] * rstd) * ga[1], (a[2] * rstd) * ga[2], (a[3] * rstd) * ga[3],
                      (b[0] * rstd) * gb[0], (b[1] * rstd) * gb[1], (b[2] * rstd) * gb[2], (b[3] * rstd) * gb[3]};
        if (SHIFT) {
            o[0] += sa[0], o[1] += sa[1], o[2] += sa[2], o[3] += sa[3], o[4] += sb[0], o[5] += sb[1], o[6] += sb[2], o[7] += sb[3];
        }
        const uint4 pk = make_uint4(pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]), pack_bf2(o[4], o[5]), pack_bf2(o[6], o[7]));
        if constexpr (!MXQ) {
            *reinterpret_cast<uint4*>(yr + c) = pk;
        } else {
            const float v[8] = {bf_lo(pk.x), bf_hi(pk.x), bf_lo(pk.y), bf_hi(pk.y), bf_lo(pk.z), bf_hi(pk.z), bf_lo(pk.w), bf_hi(pk.w)};
            float amax = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(v[e]));
            amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
            amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
            const int sbe = mx_block_exp(amax);
            const float inv = __uint_as_float((uint32_t)(254 - sbe) << 23);
            uint8_t* qr = reinterpret_cast<uint8_t*>(y) + (long)row * D + c;
            *reinterpret_cast<uint2*>(qr) = make_uint2(mx_pack4(v[0], v[1], v[2], v[3], inv), mx_pack4(v[4], v[5], v[6], v[7], inv));
            uint32_t wv = (uint32_t)sbe << (8 * ((lane >> 2) & 3));  // lanes 4b..4b+3 = block b of the 16-lane (128-column) K step
            wv |= __shfl_xor(wv, 4, 64);
            wv |= __shfl_xor(wv, 8, 64);
            if ((lane & 15) == 0) mxs[(long)(c >> 7) * mx_pad + row] = wv;
        }
    };
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    if (NP > 0) {
        // every load of the row - x and the (cached) per-column vectors - is requested before the reduction: with the vector
        // loads left after it, and a run-time `if (shift)` between them, each pass paid its own L2 round trip
        f32x4 xa[NP > 0 ? NP : 1], xb[NP > 0 ? NP : 1], ga[NP > 0 ? NP : 1], gb[NP > 0 ? NP : 1], sa[NP > 0 ? NP : 1], sb[NP > 0 ? NP : 1];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            xa[p] = *reinterpret_cast<const f32x4*>(xr + p * 512 + lane * 8);
            xb[p] = *reinterpret_cast<const f32x4*>(xr + p * 512 + lane * 8 + 4);
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            ga[p] = *reinterpret_cast<const f32x4*>(gp + p * 512 + lane * 8);
            gb[p] = *reinterpret_cast<const f32x4*>(gp + p * 512 + lane * 8 + 4);
            sa[p] = SHIFT ? *reinterpret_cast<const f32x4*>(sp + p * 512 + lane * 8) : z4;
            sb[p] = SHIFT ? *reinterpret_cast<const f32x4*>(sp + p * 512 + lane * 8 + 4) : z4;
        }
        float ss = 0.f;
#pragma unroll
        for (int p = 0; p < NP; ++p)
            ss += xa[p][0] * xa[p][0] + xa[p][1] * xa[p][1] + xa[p][2] * xa[p][2] + xa[p][3] * xa[p][3] + xb[p][0] * xb[p][0] +
                  xb[p][1] * xb[p][1] + xb[p][2] * xb[p][2] + xb[p][3] * xb[p][3];
        ss = wave_sum(ss);
        const float rstd = rsqrtf(ss / (float)D + eps);
#pragma unroll
        for (int p = 0; p < NP; ++p) emit(p * 512 + lane * 8, xa[p], xb[p], ga[p], gb[p], sa[p], sb[p], rstd);
    } else {
        float ss = 0.f;
        for (int c = lane * 8; c < D; c += 512) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(xr + c), b = *reinterpret_cast<const f32x4*>(xr + c + 4);
            ss += a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3] + b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3];
        }
        ss = wave_sum(ss);
        const float rstd = rsqrtf(ss / (float)D + eps);
        for (int c = lane * 8; c < D; c += 512)
            emit(c, *reinterpret_cast<const f32x4*>(xr + c), *reinterpret_cast<const f32x4*>(xr + c + 4), *reinterpret_cast<const f32x4*>(gp + c),
                 *reinterpret_cast<const f32x4*>(gp + c + 4), SHIFT ? *reinterpret_cast<const f32x4*>(sp + c) : z4,
                 SHIFT ? *reinterpret_cast<const f32x4*>(sp + c + 4) : z4, rstd);
    }
}
// g / sft of every modulated norm of a forward in one launch.  entries[e] = {w, sc1, sh1, sc2_off, sh2_off}: the per-step
// halves come from tproj[row * tp_stride + off + c].  out[(row * n_entries + e) * 2 * D + {0, D} + c].
__global__ void mod_gs_kernel(const ModEntry* __restrict__ entries, int n_entries, const float* __restrict__ tproj, long tp_stride,
                              float* __restrict__ out, int D) {
    const int e = blockIdx.x, row = blockIdx.y;
    const ModEntry me = entries[e];
    const float* tp = tproj + (long)row * tp_stride;
    float* o = out + ((long)row * n_entries + e) * 2 * D;
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
        o[c] = me.w[c] * (1.f + (me.sc1[c] + tp[me.sc2_off + c]));
        o[D + c] = me.sh1[c] + tp[me.sh2_off + c];
    }
}

// Folded RMSNorm (dit.hip): the shift rows of every modulated norm as bf16 GEMM operands, out[e][row][D] <- gs[row][e][1][D]
__global__ void shift_rows_kernel(const float* __restrict__ gs, int n_entries, int rows, bf16_t* __restrict__ out, int D) {
    const int e = blockIdx.x, row = blockIdx.y;
    const float* src = gs + ((long)row * n_entries + e) * 2 * D + D;
    bf16_t* o = out + ((long)e * rows + row) * D;
    for (int c = threadIdx.x; c < D; c += blockDim.x) o[c] = f2bf(src[c]);
}

// ------------------------------------------------------------------------------------------------
// In-place per-head RMSNorm(128) (+ RoPE, rotate-half form) on bf16 x[M, ld], heads at col0 + h*128.
// 16 lanes per head: lane j holds d = 4j..4j+3 and 64+4j..64+4j+3 (the rotate_half partners).
__global__ __launch_bounds__(256) void headnorm_rope_kernel(bf16_t* __restrict__ x, int M, int ld, int col0, int heads,
                                                            const float* __restrict__ w, const float* __restrict__ w2, int split,
                                                            float eps,
                                                            const float* __restrict__ cos_tab,
                                                            const float* __restrict__ sin_tab, int S, int paired) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const long unit = gid >> 4;  // (row, head)
    const int j = threadIdx.x & 15;
    const long total = (long)M * heads;
    const bool ok = unit < total;
    const int row = ok ? (int)(unit / heads) : 0;
    const int head = ok ? (int)(unit - (long)row * heads) : 0;
    // paired layout (PACK_ROWS_HEADPAIR projections): dims d and d+64 sit in columns 2d and 2d+1, so lane j's eight values
    // are one 16-byte access; the arithmetic below is the same in both layouts
    bf16_t* p = x + (long)row * ld + col0 + head * 128 + (paired ? j * 8 : j * 4);
    uint2 lo = make_uint2(0, 0), hi = make_uint2(0, 0);
    float a[4], b[4];
    if (paired) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (ok) v = *reinterpret_cast<const uint4*>(p);
        a[0] = bf_lo(v.x), b[0] = bf_hi(v.x), a[1] = bf_lo(v.y), b[1] = bf_hi(v.y);
        a[2] = bf_lo(v.z), b[2] = bf_hi(v.z), a[3] = bf_lo(v.w), b[3] = bf_hi(v.w);
    } else {
        if (ok) {
            lo = *reinterpret_cast<const uint2*>(p);
            hi = *reinterpret_cast<const uint2*>(p + 64);
        }
        a[0] = bf_lo(lo.x), a[1] = bf_hi(lo.x), a[2] = bf_lo(lo.y), a[3] = bf_hi(lo.y);
        b[0] = bf_lo(hi.x), b[1] = bf_hi(hi.x), b[2] = bf_lo(hi.y), b[3] = bf_hi(hi.y);
    }
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) ss += a[e] * a[e] + b[e] * b[e];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float rstd = rsqrtf(ss * (1.f / 128.f) + eps);
    const float* wp = (head >= split) ? w2 : w;  // heads [0,split) use w (q_norm), the rest w2 (k_norm)
    const float4 wl = *reinterpret_cast<const float4*>(wp + j * 4);
    const float4 wh = *reinterpret_cast<const float4*>(wp + 64 + j * 4);
    a[0] = wl.x * (a[0] * rstd); a[1] = wl.y * (a[1] * rstd); a[2] = wl.z * (a[2] * rstd); a[3] = wl.w * (a[3] * rstd);
    b[0] = wh.x * (b[0] * rstd); b[1] = wh.y * (b[1] * rstd); b[2] = wh.z * (b[2] * rstd); b[3] = wh.w * (b[3] * rstd);
    if (cos_tab) {
        const int pos = row % S;
        const float4 c = *reinterpret_cast<const float4*>(cos_tab + (long)pos * 64 + j * 4);
        const float4 s = *reinterpret_cast<const float4*>(sin_tab + (long)pos * 64 + j * 4);
        const float cc[4] = {c.x, c.y, c.z, c.w}, sn[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float lo_ = a[e] * cc[e] - b[e] * sn[e];
            const float hi_ = b[e] * cc[e] + a[e] * sn[e];
            a[e] = lo_;
            b[e] = hi_;
        }
    }
    if (ok && paired) {
        *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf2(a[0], b[0]), pack_bf2(a[1], b[1]), pack_bf2(a[2], b[2]), pack_bf2(a[3], b[3]));
    } else if (ok) {
        *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf2(a[0], a[1]), pack_bf2(a[2], a[3]));
        *reinterpret_cast<uint2*>(p + 64) = make_uint2(pack_bf2(b[0], b[1]), pack_bf2(b[2], b[3]));
    }
}

// ------------------------------------------------------------------------------------------------
// vt[n][h][d][s] = x[(n*S + s)*ld + col0 + h*128 + d]; pad keys s in [S, s_pad) are written as zero.
__global__ __launch_bounds__(256) void transpose_v_kernel(const bf16_t* __restrict__ x, int ld, int col0, int S, int heads,
                                                          bf16_t* __restrict__ vt, int s_pad) {
    // 16-byte chunks of a row are XOR-swizzled with (key >> 3): the transposed reads below walk keys 8 apart, which any
    // 16-byte-aligned row pitch maps onto the same banks (the former +8 padding left them 8-way conflicted)
    __shared__ bf16_t tile[64][128];
    const int s0 = blockIdx.x * 64, h = blockIdx.y, n = blockIdx.z;
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = tid + i * 256, key = c >> 4, ch = c & 15;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (s0 + key < S) v = *reinterpret_cast<const uint4*>(x + ((long)n * S + s0 + key) * ld + col0 + h * 128 + ch * 8);
        *reinterpret_cast<uint4*>(&tile[key][(ch ^ ((key >> 3) & 7)) * 8]) = v;
    }
    __syncthreads();
    bf16_t* base = vt + ((long)n * heads + h) * 128 * s_pad;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = tid + i * 256, d = c >> 3, kc = c & 7;
        uint32_t o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {  // rows kc*8 .. kc*8+7 share (row >> 3) = kc
            const int col = (((d >> 3) ^ kc) << 3) | (d & 7);
            o[e] = (uint32_t)tile[kc * 8 + 2 * e][col] | ((uint32_t)tile[kc * 8 + 2 * e + 1][col] << 16);
        }
        if (s0 + kc * 8 < s_pad) *reinterpret_cast<uint4*>(base + (long)d * s_pad + s0 + kc * 8) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// ------------------------------------------------------------------------------------------------
// OCP MXFP8 quantiser: x bf16 [M, K] -> q fp8 e4m3 [M, K] + one E8M0 scale per 32 consecutive K elements of a row.
// Shared exponent (OCP Microscaling v1.0, 6.3): e = floor(log2(max|v|)) - emax(e4m3 = 8); elements = round-to-nearest-even of v * 2^-e,
// saturated to +-448.  Scale bytes are stored as uint32 [K / 128][rows_pad]: byte b of word [kt][row] = block 4 kt + b (what one K step
// of the MX GEMM consumes per row).  One wave per row: lane j owns block j of each 2048-column span (64 bytes in, 32 bytes out).
__global__ __launch_bounds__(256) void mx_quant_kernel(const bf16_t* __restrict__ x, long ld, int M, int K, uint8_t* __restrict__ q,
                                                       uint32_t* __restrict__ scales, int rows_pad) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    for (int k0 = 0; k0 < K; k0 += 2048) {
        const int col = k0 + lane * 32;
        const bool act = col < K;
        uint4 in[4];
        float v[32];
        float amax = 0.f;
        if (act) {
#pragma unroll
            for (int i = 0; i < 4; ++i) in[i] = *reinterpret_cast<const uint4*>(x + (long)row * ld + col + i * 8);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t w[4] = {in[i].x, in[i].y, in[i].z, in[i].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[i * 8 + 2 * e] = bf_lo(w[e]);
                    v[i * 8 + 2 * e + 1] = bf_hi(w[e]);
                }
            }
#pragma unroll
            for (int e = 0; e < 32; ++e) amax = fmaxf(amax, fabsf(v[e]));
        }
        // floor(log2(amax)) from the exponent field (bf16 inputs have no fp32 subnormals worth modelling: amax < 2^-126 -> scale 2^-127)
        const int ex = (int)((__float_as_uint(amax) >> 23) & 0xffu);          // biased exponent of amax
        int sb = ex - 8;                                                       // biased E8M0 = floor(log2 amax) - 8 + 127
        sb = sb < 0 ? 0 : (sb > 254 ? 254 : sb);
        const float inv = __uint_as_float((uint32_t)(254 - sb) << 23);        // 2^-(sb - 127)
        if (act) {
            uint32_t out[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float a0 = fminf(fmaxf(v[4 * e + 0] * inv, -448.f), 448.f), a1 = fminf(fmaxf(v[4 * e + 1] * inv, -448.f), 448.f);
                float a2 = fminf(fmaxf(v[4 * e + 2] * inv, -448.f), 448.f), a3 = fminf(fmaxf(v[4 * e + 3] * inv, -448.f), 448.f);
                int pk = __builtin_amdgcn_cvt_pk_fp8_f32(a0, a1, 0, false);
                pk = __builtin_amdgcn_cvt_pk_fp8_f32(a2, a3, pk, true);
                out[e] = (uint32_t)pk;
            }
            uint8_t* qp = q + (long)row * K + col;
            *reinterpret_cast<uint4*>(qp) = make_uint4(out[0], out[1], out[2], out[3]);
            *reinterpret_cast<uint4*>(qp + 16) = make_uint4(out[4], out[5], out[6], out[7]);
        }
        // four neighbouring lanes = the four blocks of one 128-column K step
        uint32_t wv = (uint32_t)sb << (8 * (lane & 3));
        wv |= __shfl_xor(wv, 1, 64);
        wv |= __shfl_xor(wv, 2, 64);
        if (act && (lane & 3) == 0) scales[(long)(col >> 7) * rows_pad + row] = wv;
    }
}

// ------------------------------------------------------------------------------------------------
// TimestepEmbedding.timestep_embedding (base.py:225-246): out[m][0:128] = cos(t*1000*f_k), [128:256] = sin(..)
__global__ void sinusoid_kernel(TVals tv, int n, float* __restrict__ out) {
    const int m = blockIdx.x, k = threadIdx.x;  // 128 threads
    if (m >= n) return;
    const float f = expf(-logf(10000.f) * (float)k / 128.f);
    const float a = (tv.t[m] * 1000.f) * f;
    out[m * 256 + k] = cosf(a);
    out[m * 256 + 128 + k] = sinf(a);
}

// out[m][n] (+)= sum_k in[m][k] * W[n][k] + b[n]; optional second output silu(value) (own value, not accumulated)
// one wave per output column n, all Mr <= 16 rows at once (weights streamed exactly once).
template <int MT>
__global__ __launch_bounds__(256) void small_linear_kernel(const float* __restrict__ in, const bf16_t* __restrict__ W,
                                                           const float* __restrict__ b, float* __restrict__ out,
                                                           float* __restrict__ out_silu, int Mr, int N, int K,
                                                           int silu_out, int accumulate) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (n >= N) return;
    float acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = 0.f;
    const bf16_t* wr = W + (long)n * K;
    for (int k0 = lane * 8; k0 < K; k0 += 512) {
        const uint4 wv = *reinterpret_cast<const uint4*>(wr + k0);
        const float wf[8] = {bf_lo(wv.x), bf_hi(wv.x), bf_lo(wv.y), bf_hi(wv.y), bf_lo(wv.z), bf_hi(wv.z), bf_lo(wv.w), bf_hi(wv.w)};
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < Mr) {
                const float4 x0 = *reinterpret_cast<const float4*>(in + (long)m * K + k0);
                const float4 x1 = *reinterpret_cast<const float4*>(in + (long)m * K + k0 + 4);
                acc[m] += wf[0] * x0.x + wf[1] * x0.y + wf[2] * x0.z + wf[3] * x0.w + wf[4] * x1.x + wf[5] * x1.y + wf[6] * x1.z + wf[7] * x1.w;
            }
        }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = wave_sum(acc[m]);
    if (lane == 0) {
        const float bias = b ? b[n] : 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < Mr) {
                float v = acc[m] + bias;
                if (out_silu) out_silu[(long)m * N + n] = silu_f(v);
                if (silu_out) v = silu_f(v);
                float* o = out + (long)m * N + n;
                *o = accumulate ? (*o + v) : v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// xin[n][t][0:128] = bf16(ctx[n][t][:]), xin[n][t][128:192] = bf16(x[n][t][:]); rows t in [T, Tpad) are zero.
__global__ void pack_xin_kernel(const float* __restrict__ x, const float* __restrict__ ctx, bf16_t* __restrict__ xin,
                                int T, int Tpad, long total /* N*Tpad*48 */) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // one thread = 4 channels
    if (i >= total) return;
    const int q = (int)(i % 48);
    const long row = i / 48;
    const int t = (int)(row % Tpad);
    const long n = row / Tpad;
    const bool is_ctx = q < 32;
    const float* src = is_ctx ? ctx : x;
    if (!src) return;  // this part of the row is owned by another call
    float4 v = make_float4(0, 0, 0, 0);
    if (t < T) v = is_ctx ? *reinterpret_cast<const float4*>(ctx + (n * T + t) * 128 + q * 4)
                          : *reinterpret_cast<const float4*>(x + (n * T + t) * 64 + (q - 32) * 4);
    *reinterpret_cast<uint2*>(xin + row * 192 + q * 4) = make_uint2(pack_bf2(v.x, v.y), pack_bf2(v.z, v.w));
}

__global__ void f32_to_bf16_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, long n) {
    const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 3 < n) {
        const float4 v = *reinterpret_cast<const float4*>(in + i);
        *reinterpret_cast<uint2*>(out + i) = make_uint2(pack_bf2(v.x, v.y), pack_bf2(v.z, v.w));
    } else {
        for (long j = i; j < n; ++j) out[j] = f2bf(in[j]);
    }
}

__global__ void bcast_rows_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out, int rows, int cols) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)rows * cols) return;
    out[i] = in[i % cols];
}

// attention output row of a sequence whose keys are all identical: out[h*128+d] = v[(h / group)*128 + d]
__global__ void expand_kv_heads_kernel(const bf16_t* __restrict__ v_row, bf16_t* __restrict__ out, int hq, int hkv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hq * 128) return;
    const int h = i >> 7, d = i & 127;
    out[i] = v_row[(h / (hq / hkv)) * 128 + d];
}

__global__ void copy_v_kernel(const float* __restrict__ vpad, float* __restrict__ v, int T, int Tpad, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // float4 units: N*T*16
    if (i >= total) return;
    const int q = (int)(i & 15);
    const long row = i >> 4;
    const int t = (int)(row % T);
    const long n = row / T;
    *reinterpret_cast<float4*>(v + row * 64 + q * 4) = *reinterpret_cast<const float4*>(vpad + (n * Tpad + t) * 64 + q * 4);
}

// ------------------------------------------------------------------------------------------------
// One sampler step after the decoder forward (base.py:1946-1979 + apg_guidance.py:33-56):
//   diff = cond - uncond; avg = diff + (-0.75) * avg_prev; d = avg * min(1, 2.5/||avg||_T)
//   (fp64) u = cond/||cond||_T; orth = d - (d.u) u;  v = cond + (g-1) orth;  xt -= v * dt
// reductions are over the T axis per (item, channel).  grid (B, 16), block 256 = 4 channels x 64 t-slices.
__global__ __launch_bounds__(256) void apg_euler_kernel(const float* __restrict__ v, long uncond_off, float* __restrict__ avg,
                                                        float* __restrict__ xt, bf16_t* __restrict__ xin, int copies, int B,
                                                        int T, int Tpad, float guidance, float dt, int apply_cfg, int do_cfg,
                                                        int first, StepUpdate up) {
    // block = CL channels x TS time slices: 4 x 64 spreads an item over 16 workgroups (B x 16 on the chip instead of B x 4;
    // the kernel is a chain of three latency-bound passes over T, 87 -> ~30 us per step at B = 8)
    constexpr int CL = 4, TS = 64;
    __shared__ double red[3][TS][CL];
    __shared__ double tot[3][CL];
    const int b = blockIdx.x, cl = threadIdx.x % CL, ts = threadIdx.x / CL;
    const int c = blockIdx.y * CL + cl;
    const float* vc = v + (long)b * Tpad * 64 + c;
    const float* vu = vc + uncond_off;
    float* av = avg + (long)b * T * 64 + c;
    float* x = xt + (long)b * T * 64 + c;
    const bool guided = do_cfg && apply_cfg;
    double saa = 0, scc = 0, sac = 0;
    if (guided) {
        for (int t = ts; t < T; t += TS) {
            const float pc = vc[(long)t * 64], pu = vu[(long)t * 64];
            float a = pc - pu;
            if (!first) a = a + (-0.75f) * av[(long)t * 64];
            av[(long)t * 64] = a;
            saa += (double)a * a;
            scc += (double)pc * pc;
            sac += (double)a * pc;
        }
        red[0][ts][cl] = saa;
        red[1][ts][cl] = scc;
        red[2][ts][cl] = sac;
        __syncthreads();
        if (ts < 3) {
            double s = 0;
#pragma unroll
            for (int i = 0; i < TS; ++i) s += red[ts][i][cl];
            tot[ts][cl] = s;
        }
        __syncthreads();
    }
    float scale = 1.f;
    double inv_nc = 0, dotf = 0;
    if (guided) {
        const float norm_a = (float)sqrt(tot[0][cl]);
        scale = fminf(1.f, 2.5f / norm_a);
        const double nc = fmax(sqrt(tot[1][cl]), 1e-12);
        inv_nc = 1.0 / nc;
        dotf = 0;  // recomputed below from the float-rounded d to follow the reference's cast order
    }
    if (guided) {
        // dot = sum_t (double)(float)(a*scale) * (cond/nc): needs a second reduction because d is rounded to fp32 first
        double sd = 0;
        for (int t = ts; t < T; t += TS) {
            const float d = av[(long)t * 64] * scale;
            sd += (double)d * ((double)vc[(long)t * 64] * inv_nc);
        }
        __syncthreads();
        red[0][ts][cl] = sd;
        __syncthreads();
        if (ts == 0) {
            double s = 0;
#pragma unroll
            for (int i = 0; i < TS; ++i) s += red[0][i][cl];
            tot[0][cl] = s;
        }
        __syncthreads();
        dotf = tot[0][cl];
    }
    for (int t = ts; t < T; t += TS) {
        const float pc = vc[(long)t * 64];
        float vv = pc;
        if (guided) {
            const float d = av[(long)t * 64] * scale;
            const double u = (double)pc * inv_nc;
            const float orth = (float)((double)d - dotf * u);
            vv = pc + (guidance - 1.f) * orth;
        }
        float xn;
        if (up.sde_noise) {  // base.py:1968-1973: x0 = x - v*t_curr; x = t_next*noise + (1 - t_next)*x0
            const float x0 = x[(long)t * 64] - vv * up.t_curr;
            xn = up.t_next * up.sde_noise[((long)b * T + t) * 64 + c] + (1.f - up.t_next) * x0;
        } else {
            xn = x[(long)t * 64] - vv * dt;
        }
        x[(long)t * 64] = xn;
        if (xin) {
            const bf16_t xb = f2bf(xn);
            for (int cp = 0; cp < copies; ++cp) xin[((long)(cp * B + b) * Tpad + t) * 192 + 128 + c] = xb;
        }
    }
}

// ADG (apg_guidance.py:107-180, angle clip pi/6 written 3.14/6, no norm) + update; one wave per (item, frame) row of 64
// channels.  Angle / cos / sin in fp64 like the reference (`.to(float)` = float64 there); the projection in fp32.
__global__ __launch_bounds__(256) void adg_step_kernel(const float* __restrict__ v, long uncond_off, float* __restrict__ xt,
                                                       bf16_t* __restrict__ xin, int copies, int B, int T, int Tpad, float guidance,
                                                       float sigma, float dt, StepUpdate up) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int c = threadIdx.x & 63;
    if (row >= (long)B * T) return;
    const int b = (int)(row / T), t = (int)(row - (long)b * T);
    const float pc = v[((long)b * Tpad + t) * 64 + c], pu = v[uncond_off + ((long)b * Tpad + t) * 64 + c];
    const float x = xt[row * 64 + c];
    float w = guidance - 1.f;
    w = w * (w > 0.f ? 1.f : 0.f) + 1e-3f;
    const float xtxt = x - sigma * pc, xunc = x - sigma * pu, diff = xtxt - xunc;
    const double ntt = wave_sum_d((double)xtxt * xtxt), nuu = wave_sum_d((double)xunc * xunc), dtu = wave_sum_d((double)xtxt * xunc);
    double cosv = dtu / (sqrt(ntt) * sqrt(nuu));
    const double theta = acos(cosv);
    const double clipv = 3.14 / 6;
    const double th_new = fmin(fmax((double)w * theta, -clipv), clipv);
    const float du = wave_sum(diff * xunc), uu = wave_sum(xunc * xunc);
    const float perp = diff - (du / (uu + 1e-8f)) * xunc;
    const double sth = sin(theta);
    const double pnew = (sth > 1e-3) ? (double)perp * sin(th_new) / sth : (double)perp * (double)w;
    const double xnew = cos(th_new) * (double)xtxt + pnew;
    const float vv = (float)(((double)x - xnew) / (double)sigma);
    float xn;
    if (up.sde_noise) {
        const float x0 = x - vv * up.t_curr;
        xn = up.t_next * up.sde_noise[row * 64 + c] + (1.f - up.t_next) * x0;
    } else {
        xn = x - vv * dt;
    }
    xt[row * 64 + c] = xn;
    if (xin) {
        const bf16_t xb = f2bf(xn);
        for (int cp = 0; cp < copies; ++cp) xin[((long)(cp * B + b) * Tpad + t) * 192 + 128 + c] = xb;
    }
}

// ------------------------------------------------------------------------------------------------
__global__ void absmax_kernel(const float* __restrict__ wav, long per_item, float* __restrict__ peaks) {
    const int b = blockIdx.y;
    const float* p = wav + (long)b * per_item;
    float m = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < per_item; i += (long)gridDim.x * blockDim.x) m = fmaxf(m, fabsf(p[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned int*>(peaks + b), __float_as_uint(m));  // m >= 0
}
__global__ void peak_scale_kernel(float* __restrict__ wav, long per_item, int B, const float* __restrict__ peaks) {
    bool any = false;
    for (int i = 0; i < B; ++i) any |= peaks[i] > 1.f;
    if (!any) return;
    const int b = blockIdx.y;
    const float inv = 1.f / fmaxf(peaks[b], 1.f);
    float* p = wav + (long)b * per_item;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < per_item; i += (long)gridDim.x * blockDim.x) p[i] *= inv;
}
// normalize_audio (acestep/audio_utils.py:24-62): gain = fp32(10^(dB/20)) * (1 / peak) exactly as torch evaluates
// `target_amp / peak` (Tensor.__rtruediv__ = reciprocal * scalar); items with peak < 1e-6 stay untouched.
__global__ void normalize_db_kernel(float* __restrict__ wav, long per_item, float amp, const float* __restrict__ peaks) {
    const int b = blockIdx.y;
    const float peak = peaks[b];
    if (peak < 1e-6f) return;
    const float gain = __fmul_rn(1.0f / peak, amp);  // correctly rounded divide (hipcc default), as torch.reciprocal
    float* p = wav + (long)b * per_item;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < per_item; i += (long)gridDim.x * blockDim.x) p[i] = __fmul_rn(p[i], gain);
}
// [items][C][S] f32 -> [items][S][C] int16, lrintf(x * 32767) (libsndfile's float -> PCM_16 rule, round half to even),
// saturated.  C <= 8; 8 frames per thread so both the loads (per channel) and the store stream are contiguous.
template <int C>
__global__ void pcm16_interleave_kernel(const float* __restrict__ wav, long S, int16_t* __restrict__ out) {
    const int b = blockIdx.y;
    const float* p = wav + (long)b * C * S;
    int16_t* o = out + (long)b * C * S;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += (long)gridDim.x * blockDim.x) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int v = __float2int_rn(__fmul_rn(p[(long)c * S + i], 32767.f));
            o[i * C + c] = (int16_t)(v > 32767 ? 32767 : (v < -32768 ? -32768 : v));
        }
    }
}
template <int C>
__global__ void f32_interleave_kernel(const float* __restrict__ wav, long S, float* __restrict__ out) {
    const int b = blockIdx.y;
    const float* p = wav + (long)b * C * S;
    float* o = out + (long)b * C * S;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += (long)gridDim.x * blockDim.x) {
#pragma unroll
        for (int c = 0; c < C; ++c) o[i * C + c] = p[(long)c * S + i];
    }
}
__global__ void latent_check_kernel(const float* __restrict__ x, long n, int* __restrict__ flags) {
    bool bad = false, nz = false;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float v = x[i];
        bad |= !(fabsf(v) <= 3.0e38f);
        nz |= (v != 0.f);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flags, 1);
    if (__any(nz) && (threadIdx.x & 63) == 0) atomicOr(flags + 1, 1);
}

// ------------------------------------------------------------------------------------------------
template <typename SRC>
__device__ __forceinline__ float ldsrc(const SRC* p, long i);
template <>
__device__ __forceinline__ float ldsrc<float>(const float* p, long i) { return p[i]; }
template <>
__device__ __forceinline__ float ldsrc<bf16_t>(const bf16_t* p, long i) { return bf2f(p[i]); }

template <typename SRC>
__global__ void pack_kernel(const SRC* __restrict__ src, void* __restrict__ dst, int dst_is_bf16, int mode, long rows, long cols,
                            long dst_ld, long dst_row0, int p0, int p1) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cols) return;
    const long r = i / cols, c = i - r * cols;
    long di;
    if (mode == PACK_ROWS || mode == PACK_ROWS_IL32 || mode == PACK_ROWS_HEADPAIR) {
        di = pack_row(mode, r, dst_row0, p0) * dst_ld + c;
    } else if (mode == PACK_CONV_IN) {  // src [O][C][P] -> dst[o][p*C + c]
        const long cc = c / p1, pp = c - cc * p1;
        di = (dst_row0 + r) * dst_ld + pp * p0 + cc;
    } else {  // PACK_CONVT_OUT: src [I][C][P] -> dst[p*C + c][i]
        const long cc = c / p1, pp = c - cc * p1;
        di = (dst_row0 + pp * p0 + cc) * dst_ld + r;
    }
    const float v = ldsrc<SRC>(src, i);
    if (dst_is_bf16) reinterpret_cast<bf16_t*>(dst)[di] = f2bf(v);
    else reinterpret_cast<float*>(dst)[di] = v;
}

// zero fill of integer accumulators that device-scope atomics add into (the folded norms' row sums, dit.hip forward_core)
__global__ void zero_u64_kernel(unsigned long long* __restrict__ p, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0ull;
}

// mean over the sequence of every V head channel (fully-masked attention rows of the condition encoders, see AttnArgs::vmean)
__global__ void vmean_kernel(const bf16_t* __restrict__ x, int ld, int col0, int S, bf16_t* __restrict__ out, int heads) {
    const int h = blockIdx.x, n = blockIdx.y, d = threadIdx.x;
    const bf16_t* p = x + (long)n * S * ld + col0 + h * 128 + d;
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc += bf2f(p[(long)s * ld]);
    out[((long)n * heads + h) * 128 + d] = f2bf(acc / (float)S);
}

__global__ void gather_rows_bf16_f32_kernel(const bf16_t* __restrict__ src, long src_ld, const int* __restrict__ row_src,
                                            float* __restrict__ dst, long dst_ld, long rows, int cols) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c4 = cols / 4;
    if (i >= rows * c4) return;
    const long r = i / c4;
    const int c = (int)(i - r * c4) * 4;
    const int sr = row_src[r];
    if (sr < -1) return;  // row owned by another source buffer
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (sr >= 0) {
        const uint2 u = *reinterpret_cast<const uint2*>(src + (long)sr * src_ld + c);
        v = {bf_lo(u.x), bf_hi(u.x), bf_lo(u.y), bf_hi(u.y)};
    }
    *reinterpret_cast<float4*>(dst + r * dst_ld + c) = v;
}

// AudioTokenDetokenizer (base.py:889-894): h[(r*P + p)][c] = emb[r][c] + special[p][c]
__global__ void expand_add_kernel(const float* __restrict__ emb, const float* __restrict__ special, float* __restrict__ out, long rows,
                                  int P, int D) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int d4 = D / 4;
    if (i >= rows * P * d4) return;
    const long rp = i / d4;
    const int c = (int)(i - rp * d4) * 4;
    const long r = rp / P;
    const int p = (int)(rp - r * P);
    const float4 a = *reinterpret_cast<const float4*>(emb + r * D + c);
    const float4 b = *reinterpret_cast<const float4*>(special + (long)p * D + c);
    *reinterpret_cast<float4*>(out + rp * D + c) = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// AceStepAudioTokenizer helpers (cond.hip: ace355_tok_run).  pad_rows: f32 [rows, cols] -> bf16 [rows, ld] with zeros beyond `cols`.
__global__ void pad_rows_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ out, long rows, int cols, int ld) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * ld) return;
    const long r = i / ld;
    const int c = (int)(i - r * ld);
    out[i] = c < cols ? f2bf(x[r * cols + c]) : (bf16_t)0;
}
// AttentionPooler (base.py:769-771): out[r * (P + 1)] = special, out[r * (P + 1) + 1 + p] = emb[r * P + p]
__global__ void prepend_special_kernel(const float* __restrict__ emb, const float* __restrict__ special, float* __restrict__ out, long rows,
                                       int P, int D) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int d4 = D / 4;
    if (i >= rows * (P + 1) * d4) return;
    const long rp = i / d4;
    const int c = (int)(i - rp * d4) * 4;
    const long r = rp / (P + 1);
    const int p = (int)(rp - r * (P + 1));
    const float4 v = p == 0 ? *reinterpret_cast<const float4*>(special + c) : *reinterpret_cast<const float4*>(emb + (r * P + p - 1) * D + c);
    *reinterpret_cast<float4*>(out + rp * D + c) = v;
}
// pooled output (base.py:856-858): out[r][:] = f32(x[r * S][:])
__global__ void take_token0_kernel(const bf16_t* __restrict__ x, float* __restrict__ out, long rows, int S, int D) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * D) return;
    const long r = i / D;
    out[i] = bf2f(x[r * S * D + (i - r * D)]);
}

inline int blocks_for(long n, int per) { return (int)((n + per - 1) / per); }

}  // namespace

int launch_rmsnorm_mod(const float* x, const float* w, bf16_t* y, int M, int D, float eps, const float* sc1,
                       const float* sc2, const float* sh1, const float* sh2, int stride, int rows_per_seq, hipStream_t s) {
    ACE_CHECK(D % 4 == 0, "rmsnorm: D % 4");
    ACE_CHECK(!sc1 || (sc2 && sh1 && sh2 && rows_per_seq > 0), "rmsnorm: modulation needs all four vectors");
    const int rps = rows_per_seq > 0 ? rows_per_seq : 1;
    if (!sc1 && D % 8 == 0) return launch_rmsnorm_gs(x, w, nullptr, y, M, D, eps, 0, rps, s);
    if (D == 2048) hipLaunchKernelGGL(rmsnorm_mod_kernel<8>, dim3((M + 3) / 4), dim3(256), 0, s, x, w, y, M, D, eps, sc1, sc2, sh1, sh2, stride, rps);
    else if (D == 256) hipLaunchKernelGGL(rmsnorm_mod_kernel<1>, dim3((M + 3) / 4), dim3(256), 0, s, x, w, y, M, D, eps, sc1, sc2, sh1, sh2, stride, rps);
    else hipLaunchKernelGGL(rmsnorm_mod_kernel<0>, dim3((M + 3) / 4), dim3(256), 0, s, x, w, y, M, D, eps, sc1, sc2, sh1, sh2, stride, rps);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_rmsnorm_gs_mx(const float* x, const float* g, const float* sft, uint8_t* q, uint32_t* scales, int rows_pad, int M, int D,
                         float eps, long stride, int rows_per_seq, hipStream_t s) {
    ACE_CHECK(D == 2048 && stride % 4 == 0 && rows_pad >= M, "rmsnorm_gs_mx: D = 2048 only");
    const int rps = rows_per_seq > 0 ? rows_per_seq : 1;
    const dim3 grid((M + 3) / 4);
    if (sft) hipLaunchKernelGGL((rmsnorm_gs_kernel<4, true, true>), grid, dim3(256), 0, s, x, g, sft, reinterpret_cast<bf16_t*>(q), M, D, eps, stride, rps, scales, rows_pad);
    else hipLaunchKernelGGL((rmsnorm_gs_kernel<4, false, true>), grid, dim3(256), 0, s, x, g, sft, reinterpret_cast<bf16_t*>(q), M, D, eps, stride, rps, scales, rows_pad);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_rmsnorm_gs(const float* x, const float* g, const float* sft, bf16_t* y, int M, int D, float eps, long stride,
                      int rows_per_seq, hipStream_t s) {
    ACE_CHECK(D % 8 == 0 && stride % 4 == 0, "rmsnorm_gs: D % 8, stride % 4");
    const int rps = rows_per_seq > 0 ? rows_per_seq : 1;
    const dim3 grid((M + 3) / 4);
    if (D == 2048 && sft) hipLaunchKernelGGL((rmsnorm_gs_kernel<4, true>), grid, dim3(256), 0, s, x, g, sft, y, M, D, eps, stride, rps);
    else if (D == 2048) hipLaunchKernelGGL((rmsnorm_gs_kernel<4, false>), grid, dim3(256), 0, s, x, g, sft, y, M, D, eps, stride, rps);
    else if (sft) hipLaunchKernelGGL((rmsnorm_gs_kernel<0, true>), grid, dim3(256), 0, s, x, g, sft, y, M, D, eps, stride, rps);
    else hipLaunchKernelGGL((rmsnorm_gs_kernel<0, false>), grid, dim3(256), 0, s, x, g, sft, y, M, D, eps, stride, rps);
    ACE_LAUNCH_CHECK();
    return 0;
}
int launch_mod_gs(const ModEntry* entries_dev, int n_entries, const float* tproj, long tp_stride, int rows, float* out, int D,
                  hipStream_t s) {
    hipLaunchKernelGGL(mod_gs_kernel, dim3(n_entries, rows), dim3(256), 0, s, entries_dev, n_entries, tproj, tp_stride, out, D);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_shift_rows(const float* gs, int n_entries, int rows, bf16_t* out, int D, hipStream_t s) {
    hipLaunchKernelGGL(shift_rows_kernel, dim3(n_entries, rows), dim3(256), 0, s, gs, n_entries, rows, out, D);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_vmean(const bf16_t* x, int ld, int col0, int N, int S, int heads, bf16_t* vmean, hipStream_t s) {
    hipLaunchKernelGGL(vmean_kernel, dim3(heads, N), dim3(128), 0, s, x, ld, col0, S, vmean, heads);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_gather_rows_bf16_f32(const bf16_t* src, long src_ld, const int* row_src, float* dst, long dst_ld, long rows, int cols,
                                hipStream_t s) {
    ACE_CHECK(cols % 4 == 0, "gather_rows: cols must be a multiple of 4");
    const long n = rows * (cols / 4);
    hipLaunchKernelGGL(gather_rows_bf16_f32_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, src, src_ld, row_src, dst, dst_ld, rows, cols);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_expand_add(const float* emb, const float* special, float* out, long rows, int P, int D, hipStream_t s) {
    ACE_CHECK(D % 4 == 0, "expand_add: D must be a multiple of 4");
    const long n = rows * P * (D / 4);
    hipLaunchKernelGGL(expand_add_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, emb, special, out, rows, P, D);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_pad_rows_bf16(const float* x, bf16_t* out, long rows, int cols, int ld, hipStream_t s) {
    hipLaunchKernelGGL(pad_rows_bf16_kernel, dim3(blocks_for(rows * ld, 256)), dim3(256), 0, s, x, out, rows, cols, ld);
    ACE_LAUNCH_CHECK();
    return 0;
}
int launch_prepend_special(const float* emb, const float* special, float* out, long rows, int P, int D, hipStream_t s) {
    ACE_CHECK(D % 4 == 0, "prepend_special: D must be a multiple of 4");
    hipLaunchKernelGGL(prepend_special_kernel, dim3(blocks_for(rows * (P + 1) * (D / 4), 256)), dim3(256), 0, s, emb, special, out, rows, P, D);
    ACE_LAUNCH_CHECK();
    return 0;
}
// out[m][n] = sum_k x[m][k] W[n][k] + b[n], everything fp32 (fp64 accumulation: the caller rounds the result to FSQ digits, and a
// half-way case must not depend on a summation order).  The two projections of the residual FSQ on the LM-hint path (K = 6 -> hidden and
// hidden -> 6; lmhints.py): K <= 64: one lane per output element, else one wave per output element (lanes stride K, butterfly sum).
__global__ __launch_bounds__(256) void linear_f32_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ b,
                                                         float* __restrict__ out, long M, int N, int K) {
    if (K <= 64) {
        const long i = (long)blockIdx.x * 256 + threadIdx.x;
        if (i >= M * N) return;
        const long m = i / N;
        const int n = (int)(i - m * N);
        double acc = 0.0;
        for (int k = 0; k < K; ++k) acc += (double)x[m * K + k] * (double)W[(long)n * K + k];
        out[i] = (float)(acc + (b ? (double)b[n] : 0.0));
        return;
    }
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);   // one wave per output element
    const int lane = threadIdx.x & 63;
    if (i >= M * N) return;
    const long m = i / N;
    const int n = (int)(i - m * N);
    double acc = 0.0;
    for (int k = lane; k < K; k += 64) acc += (double)x[m * K + k] * (double)W[(long)n * K + k];
    acc = wave_sum_d(acc);
    if (lane == 0) out[i] = (float)(acc + (b ? (double)b[n] : 0.0));
}
int launch_linear_f32(const float* x, const float* W, const float* b, float* out, long M, int N, int K, hipStream_t s) {
    ACE_CHECK(M > 0 && N > 0 && K > 0 && M * (long)N < (1L << 31), "linear_f32: sizes");
    const long outs = M * N;
    const long blocks = K <= 64 ? blocks_for(outs, 256) : (outs + 3) / 4;
    hipLaunchKernelGGL(linear_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, W, b, out, M, N, K);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_take_token0(const bf16_t* x, float* out, long rows, int S, int D, hipStream_t s) {
    hipLaunchKernelGGL(take_token0_kernel, dim3(blocks_for(rows * D, 256)), dim3(256), 0, s, x, out, rows, S, D);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_headnorm_rope2(bf16_t* x, int M, int ld, int col0, int heads, const float* w, const float* w2, int split, float eps,
                          const float* cos_tab, const float* sin_tab, int S, hipStream_t s, int paired) {
    ACE_CHECK(!paired || (ld % 8 == 0 && col0 % 8 == 0), "headnorm_rope: the paired layout uses 16-byte accesses");
    const long threads = (long)M * heads * 16;
    hipLaunchKernelGGL(headnorm_rope_kernel, dim3(blocks_for(threads, 256)), dim3(256), 0, s, x, M, ld, col0, heads, w, w2, split, eps,
                       cos_tab, sin_tab, S > 0 ? S : 1, paired);
    ACE_LAUNCH_CHECK();
    return 0;
}
int launch_headnorm_rope(bf16_t* x, int M, int ld, int col0, int heads, const float* w, float eps, const float* cos_tab,
                         const float* sin_tab, int S, hipStream_t s) {
    const long threads = (long)M * heads * 16;
    hipLaunchKernelGGL(headnorm_rope_kernel, dim3(blocks_for(threads, 256)), dim3(256), 0, s, x, M, ld, col0, heads, w, w, heads, eps,
                       cos_tab, sin_tab, S > 0 ? S : 1, 0);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_transpose_v(const bf16_t* x, int ld, int col0, int N, int S, int heads, bf16_t* vt, int s_pad, hipStream_t s) {
    ACE_CHECK(s_pad % 64 == 0 && s_pad >= S, "transpose_v: s_pad");
    hipLaunchKernelGGL(transpose_v_kernel, dim3(s_pad / 64, heads, N), dim3(256), 0, s, x, ld, col0, S, heads, vt, s_pad);
    ACE_LAUNCH_CHECK();
    return 0;
}

// Qwen3RotaryEmbedding (default rope): inv_freq = theta^(-2k/128) in fp32, angle = pos * inv_freq in fp32.
int launch_mx_quant(const bf16_t* x, long ld, int M, int K, uint8_t* q, uint32_t* scales, int rows_pad, hipStream_t s) {
    ACE_CHECK(K % 128 == 0 && ld % 8 == 0 && rows_pad >= M, "mx_quant: K % 128, 16-byte rows, rows_pad >= M");
    ACE_CHECK((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(q) & 15) == 0, "mx_quant: 16-byte aligned buffers");
    hipLaunchKernelGGL(mx_quant_kernel, dim3((M + 3) / 4), dim3(256), 0, s, x, ld, M, K, q, scales, rows_pad);
    ACE_LAUNCH_CHECK();
    return 0;
}

// fp8 weight-only semantics (the reference's `quantization="fp8_weight_only"`: torchao Float8WeightOnlyConfig, handler/
// init_service_loader.py:95-97): every Linear weight is held as e4m3 with one fp32 scale per output channel and dequantised to the
// activation dtype for the matmul.  There is no MFMA for bf16 x fp8, so the numerics are applied to the packed bf16 weights in place:
// w[n][:] <- bf16( e4m3_rne( w[n][:] / s_n ) * s_n ),  s_n = max(amax_n, 1e-12) / 448.  One wave per row.
__global__ __launch_bounds__(256) void fp8_weight_roundtrip_kernel(bf16_t* __restrict__ w, long ld, int N, int K) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    bf16_t* wr = w + (long)row * ld;
    float amax = 0.f;
    for (int c = lane * 2; c < K; c += 128) {
        const uint32_t p = *reinterpret_cast<const uint32_t*>(wr + c);
        amax = fmaxf(amax, fmaxf(fabsf(bf_lo(p)), fabsf(bf_hi(p))));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    const float scale = fmaxf(amax, 1e-12f) / 448.f;
    for (int c = lane * 2; c < K; c += 128) {
        const uint32_t p = *reinterpret_cast<const uint32_t*>(wr + c);
        const float a0 = fminf(fmaxf(bf_lo(p) / scale, -448.f), 448.f), a1 = fminf(fmaxf(bf_hi(p) / scale, -448.f), 448.f);
        const int pk = __builtin_amdgcn_cvt_pk_fp8_f32(a0, a1, 0, false);
        const float q0 = __builtin_amdgcn_cvt_f32_fp8(pk, 0), q1 = __builtin_amdgcn_cvt_f32_fp8(pk, 1);
        *reinterpret_cast<uint32_t*>(wr + c) = pack_bf2(q0 * scale, q1 * scale);
    }
}
int launch_fp8_weight_roundtrip(bf16_t* w, long ld, int N, int K, hipStream_t s) {
    ACE_CHECK(K % 2 == 0 && ld % 2 == 0, "fp8_weight_roundtrip: even row length");
    hipLaunchKernelGGL(fp8_weight_roundtrip_kernel, dim3((N + 3) / 4), dim3(256), 0, s, w, ld, N, K);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_rope_table(float* cos_tab, float* sin_tab, int S, float theta, hipStream_t s) {
    std::vector<float> c((size_t)S * 64), sn((size_t)S * 64);
    float inv[64];
    for (int k = 0; k < 64; ++k) inv[k] = 1.0f / powf(theta, (float)(2 * k) / 128.0f);
    for (int p = 0; p < S; ++p)
        for (int k = 0; k < 64; ++k) {
            const float a = (float)p * inv[k];
            c[(size_t)p * 64 + k] = (float)cos((double)a);
            sn[(size_t)p * 64 + k] = (float)sin((double)a);
        }
    ACE_HIP(hipMemcpyAsync(cos_tab, c.data(), c.size() * 4, hipMemcpyHostToDevice, s));
    ACE_HIP(hipMemcpyAsync(sin_tab, sn.data(), sn.size() * 4, hipMemcpyHostToDevice, s));
    ACE_HIP(hipStreamSynchronize(s));
    return 0;
}

int launch_sinusoid(const TVals& tv, int n, float* out, hipStream_t s) {
    ACE_CHECK(n <= 64, "sinusoid: n <= 64");
    hipLaunchKernelGGL(sinusoid_kernel, dim3(n), dim3(128), 0, s, tv, n, out);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_small_linear_ex(const float* in, const bf16_t* W, const float* b, float* out, float* out_silu, int Mr, int N, int K,
                           int silu_out, int accumulate, hipStream_t s) {
    ACE_CHECK(K % 8 == 0, "small_linear: K % 8");
    for (int m0 = 0; m0 < Mr; m0 += 16) {
        const int mr = Mr - m0 < 16 ? Mr - m0 : 16;
        hipLaunchKernelGGL(small_linear_kernel<16>, dim3((N + 3) / 4), dim3(256), 0, s, in + (long)m0 * K, W, b, out + (long)m0 * N,
                           out_silu ? out_silu + (long)m0 * N : nullptr, mr, N, K, silu_out, accumulate);
    }
    ACE_LAUNCH_CHECK();
    return 0;
}
int launch_small_linear(const float* in, const bf16_t* W, const float* b, float* out, int Mr, int N, int K, int silu_in,
                        int silu_out, int accumulate, hipStream_t s) {
    ACE_CHECK(!silu_in, "small_linear: silu_in is provided by the producer's second output");
    return launch_small_linear_ex(in, W, b, out, nullptr, Mr, N, K, silu_out, accumulate, s);
}

// One wave spinning on the 100 MHz wall clock: two of these on two streams take ~`us` when the streams sit on different hardware
// queues and ~2 x `us` when the runtime mapped both onto one (dit.hip: dual-chain stream probe).
__global__ void spin_kernel(unsigned long long ticks) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}
int launch_spin(int us, hipStream_t s) {
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, s, (unsigned long long)us * 100ull);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_pack_xin(const float* x, const float* ctx, bf16_t* xin, int N, int T, int Tpad, hipStream_t s) {
    const long total = (long)N * Tpad * 48;
    hipLaunchKernelGGL(pack_xin_kernel, dim3(blocks_for(total, 256)), dim3(256), 0, s, x, ctx, xin, T, Tpad, total);
    ACE_LAUNCH_CHECK();
    return 0;
}
// latent part only, replicated `copies` times along the sequence axis (CFG doubling, base.py:1929)
int launch_set_xin_latent(const float* xt, bf16_t* xin, int B, int copies, int T, int Tpad, hipStream_t s) {
    for (int cp = 0; cp < copies; ++cp) {
        int rc = launch_pack_xin(xt, nullptr, xin + (long)cp * B * Tpad * 192, B, T, Tpad, s);
        if (rc) return rc;
    }
    return 0;
}
int launch_set_xin_ctx(const float* ctx, bf16_t* xin, int B, int copies, int T, int Tpad, hipStream_t s) {
    for (int cp = 0; cp < copies; ++cp) {
        int rc = launch_pack_xin(nullptr, ctx, xin + (long)cp * B * Tpad * 192, B, T, Tpad, s);
        if (rc) return rc;
    }
    return 0;
}

int launch_f32_to_bf16(const float* in, bf16_t* out, long n, hipStream_t s) {
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(blocks_for((n + 3) / 4, 256)), dim3(256), 0, s, in, out, n);
    ACE_LAUNCH_CHECK();
    return 0;
}
int launch_expand_kv_heads(const bf16_t* v_row, bf16_t* out, int hq, int hkv, hipStream_t s) {
    hipLaunchKernelGGL(expand_kv_heads_kernel, dim3((hq * 128 + 255) / 256), dim3(256), 0, s, v_row, out, hq, hkv);
    ACE_LAUNCH_CHECK();
    return 0;
}
int launch_bcast_rows(const bf16_t* in, bf16_t* out, int rows, int cols, hipStream_t s) {
    hipLaunchKernelGGL(bcast_rows_kernel, dim3(blocks_for((long)rows * cols, 256)), dim3(256), 0, s, in, out, rows, cols);
    ACE_LAUNCH_CHECK();
    return 0;
}
int launch_copy_v(const float* vpad, float* v, int N, int T, int Tpad, hipStream_t s) {
    const long total = (long)N * T * 16;
    hipLaunchKernelGGL(copy_v_kernel, dim3(blocks_for(total, 256)), dim3(256), 0, s, vpad, v, T, Tpad, total);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_apg_euler(const float* v, long uncond_offset, float* avg, float* xt, bf16_t* xin, int copies, int B, int T, int Tpad,
                     float guidance, float dt, int apply_cfg, int do_cfg, int first, const StepUpdate& up, hipStream_t s) {
    hipLaunchKernelGGL(apg_euler_kernel, dim3(B, 16), dim3(256), 0, s, v, uncond_offset, avg, xt, xin, copies, B, T, Tpad, guidance,
                       dt, apply_cfg, do_cfg, first, up);
    ACE_LAUNCH_CHECK();
    return 0;
}
int launch_adg_step(const float* v, long uncond_offset, float* xt, bf16_t* xin, int copies, int B, int T, int Tpad, float guidance,
                    float sigma, float dt, const StepUpdate& up, hipStream_t s) {
    const long rows = (long)B * T;
    hipLaunchKernelGGL(adg_step_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, v, uncond_offset, xt, xin, copies, B, T,
                       Tpad, guidance, sigma, dt, up);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_peak_normalize(float* wav, int B, long per_item, float* scratch, hipStream_t s) {
    ACE_HIP(hipMemsetAsync(scratch, 0, sizeof(float) * B, s));
    const int gx = (int)((per_item + 256L * 16 - 1) / (256L * 16));
    const int g = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
    hipLaunchKernelGGL(absmax_kernel, dim3(g, B), dim3(256), 0, s, wav, per_item, scratch);
    hipLaunchKernelGGL(peak_scale_kernel, dim3(g, B), dim3(256), 0, s, wav, per_item, B, scratch);
    ACE_LAUNCH_CHECK();
    return 0;
}
int launch_normalize_db(float* wav, int B, long per_item, float amp, float* peaks, hipStream_t s) {
    ACE_HIP(hipMemsetAsync(peaks, 0, sizeof(float) * B, s));
    const int gx = (int)((per_item + 256L * 16 - 1) / (256L * 16));
    const int g = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
    hipLaunchKernelGGL(absmax_kernel, dim3(g, B), dim3(256), 0, s, wav, per_item, peaks);
    hipLaunchKernelGGL(normalize_db_kernel, dim3(g, B), dim3(256), 0, s, wav, per_item, amp, peaks);
    ACE_LAUNCH_CHECK();
    return 0;
}
int launch_interleave(const float* wav, int B, int C, long S, void* out, int as_pcm16, hipStream_t s) {
    const int gx = (int)((S + 255) / 256);
    const dim3 grid(gx < 1 ? 1 : (gx > 2048 ? 2048 : gx), B);
    if (C == 1) {
        if (as_pcm16) hipLaunchKernelGGL(pcm16_interleave_kernel<1>, grid, dim3(256), 0, s, wav, S, (int16_t*)out);
        else hipLaunchKernelGGL(f32_interleave_kernel<1>, grid, dim3(256), 0, s, wav, S, (float*)out);
    } else if (C == 2) {
        if (as_pcm16) hipLaunchKernelGGL(pcm16_interleave_kernel<2>, grid, dim3(256), 0, s, wav, S, (int16_t*)out);
        else hipLaunchKernelGGL(f32_interleave_kernel<2>, grid, dim3(256), 0, s, wav, S, (float*)out);
    } else {
        set_error("interleave: 1 or 2 channels");
        return 1;
    }
    ACE_LAUNCH_CHECK();
    return 0;
}
int launch_latent_check(const float* x, long n, int* flags_dev, hipStream_t s) {
    ACE_HIP(hipMemsetAsync(flags_dev, 0, 2 * sizeof(int), s));
    const int g = (int)((n + 255) / 256) > 1024 ? 1024 : (int)((n + 255) / 256);
    hipLaunchKernelGGL(latent_check_kernel, dim3(g < 1 ? 1 : g), dim3(256), 0, s, x, n, flags_dev);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_zero_u64(unsigned long long* p, long n, hipStream_t s) {
    hipLaunchKernelGGL(zero_u64_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, p, n);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_pack(const void* src, int src_dtype, void* dst, int dst_is_bf16, int mode, long rows, long cols, long dst_ld,
                long dst_row0, int p0, int p1, hipStream_t s) {
    const long n = rows * cols;
    if (src_dtype == 0)
        hipLaunchKernelGGL(pack_kernel<float>, dim3(blocks_for(n, 256)), dim3(256), 0, s, (const float*)src, dst, dst_is_bf16, mode,
                           rows, cols, dst_ld, dst_row0, p0, p1);
    else
        hipLaunchKernelGGL(pack_kernel<bf16_t>, dim3(blocks_for(n, 256)), dim3(256), 0, s, (const bf16_t*)src, dst, dst_is_bf16, mode,
                           rows, cols, dst_ld, dst_row0, p0, p1);
    ACE_LAUNCH_CHECK();
    return 0;
}

}  // namespace ace355
