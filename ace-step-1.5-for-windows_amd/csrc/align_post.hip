// align_post.hip - the lyric alignment stage after the cross-attention maps (ace355_align_*): the bidirectional-consensus filter of the
// timestamp path, the min-max energy of the score path, the DTW with its backtrace, and the three score metrics.
//
// Every kernel reads the maps as ace355_dit_cross_attention_maps wrote them, fp32 [n_pairs][N][L][S], for one item n and the lyric rows
// [row0, row0 + rows): the handlers' [layers, 16, L, S] stack is never built.  round_bf16 rounds a map value to bf16 and back on load (the
// handlers' .to(bf16) followed by the aligners' .float()).
//
// Numerics: medians are exact selections (a radix select on the order-preserving integer image of the floats, 8 bits a pass) combined as
// torch.quantile(q = 0.5) combines them; softmaxes, head means and the global mean / std accumulate in fp64; the DTW cell is the
// sequential code's own fp32 arithmetic, so its path is the sequential path, ties included.  No float atomics anywhere: the same call
// gives the same bits.  __syncthreads() is the only synchronisation between threads.
#include "common.h"

namespace ace355 {
namespace {

constexpr int TB = 256;            // threads of every kernel here but the DTW
constexpr int MED_LDS = 8192;      // a line of up to this many floats is staged in LDS for its median

__device__ __forceinline__ float ld_map(const float* p, int rb) {
    const float v = *p;
    return rb ? bf2f(f2bf(v)) : v;
}

// order-preserving float <-> uint32
__device__ __forceinline__ uint32_t f2key(float f) {
    const uint32_t b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) { return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k); }

struct RedShared {
    double d[TB / 64];
    float f[TB / 64];
};

// fixed-order block reductions (TB threads), result broadcast to every thread
__device__ double block_sum(double v, RedShared& sh) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh.d[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = sh.d[0];
    for (int w = 1; w < TB / 64; ++w) r += sh.d[w];
    return r;
}
__device__ float block_max(float v, RedShared& sh) {
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh.f[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sh.f[0];
    for (int w = 1; w < TB / 64; ++w) r = fmaxf(r, sh.f[w]);
    return r;
}
__device__ float block_min(float v, RedShared& sh) {
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_down(v, off, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh.f[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sh.f[0];
    for (int w = 1; w < TB / 64; ++w) r = fminf(r, sh.f[w]);
    return r;
}

struct SelShared {
    unsigned hist[256];
    unsigned scan[256];
    unsigned prefix, krem, cnt, mn;
};

// the key of 0-based rank k among the n floats v[i * stride] (TB == 256 threads, all of them call)
__device__ uint32_t block_kth(const float* v, size_t stride, int n, unsigned k, SelShared& sh) {
    const int t = threadIdx.x;
    uint32_t prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        sh.hist[t] = 0;
        __syncthreads();
        for (int i = t; i < n; i += TB) {
            const uint32_t key = f2key(v[(size_t)i * stride]);
            if ((key & mask) == prefix) atomicAdd(&sh.hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        const unsigned h = sh.hist[t];
        sh.scan[t] = h;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const unsigned a = t >= off ? sh.scan[t - off] : 0u;
            __syncthreads();
            sh.scan[t] += a;
            __syncthreads();
        }
        const unsigned incl = sh.scan[t], excl = incl - h;
        if (k >= excl && k < incl) {
            sh.prefix = prefix | ((uint32_t)t << shift);
            sh.krem = k - excl;
        }
        __syncthreads();
        prefix = sh.prefix;
        k = sh.krem;
        mask |= 255u << shift;
        __syncthreads();
    }
    return prefix;
}

// torch.quantile(v, 0.5) with linear interpolation: the middle order statistic, or lerp(lower, upper, 0.5) = upper - (upper - lower) * 0.5
__device__ float block_median(const float* v, size_t stride, int n, SelShared& sh) {
    const int t = threadIdx.x;
    const unsigned k1 = (unsigned)(n - 1) / 2u;
    const uint32_t key1 = block_kth(v, stride, n, k1, sh);
    const float a = key2f(key1);
    if (n & 1) return a;
    if (t == 0) { sh.cnt = 0; sh.mn = 0xffffffffu; }
    __syncthreads();
    unsigned c = 0;
    uint32_t m = 0xffffffffu;
    for (int i = t; i < n; i += TB) {
        const uint32_t key = f2key(v[(size_t)i * stride]);
        if (key <= key1) ++c; else m = min(m, key);
    }
    atomicAdd(&sh.cnt, c);
    atomicMin(&sh.mn, m);
    __syncthreads();
    const uint32_t key2 = sh.cnt >= k1 + 2u ? key1 : sh.mn;
    __syncthreads();
    const float b = key2f(key2);
    return __fsub_rn(b, __fmul_rn(__fsub_rn(b, a), 0.5f));
}

// ---------------------------------------------------------------------------------------------------------------- median test hook
// x [outer][n][inner] -> out [outer][inner], the median over n
__global__ __launch_bounds__(TB) void k_median(const float* x, int n, int inner, float* out) {
    __shared__ SelShared sh;
    __shared__ float line[MED_LDS];
    const float* v = x + (size_t)blockIdx.y * n * inner + blockIdx.x;
    float med;
    if (n <= MED_LDS) {
        for (int i = threadIdx.x; i < n; i += TB) line[i] = v[(size_t)i * inner];
        __syncthreads();
        med = block_median(line, 1, n, sh);
    } else {
        med = block_median(v, (size_t)inner, n, sh);
    }
    if (threadIdx.x == 0) out[(size_t)blockIdx.y * inner + blockIdx.x] = med;
}

// ---------------------------------------------------------------------------------------------------------------- timestamp matrix
// x(h, r, s) = maps[h * pstride + r * S + s] (maps already points at item n, row row0)

// softmax statistics over the rows of every column (h, s): max and sum of exp in fp64
__global__ __launch_bounds__(256) void k_col_stats(const float* maps, size_t pstride, int R, int S, int rb, double* cmax, double* csum) {
    __shared__ float sm[4][64];
    __shared__ double ss[4][64];
    const int tx = threadIdx.x, ty = threadIdx.y, s = blockIdx.x * 64 + tx, h = blockIdx.y;
    const float* col = maps + (size_t)h * pstride + (s < S ? s : 0);
    float m = -__builtin_inff();
    if (s < S)
        for (int r = ty; r < R; r += 4) m = fmaxf(m, ld_map(col + (size_t)r * S, rb));
    sm[ty][tx] = m;
    __syncthreads();
    m = fmaxf(fmaxf(sm[0][tx], sm[1][tx]), fmaxf(sm[2][tx], sm[3][tx]));
    double sum = 0.0;
    if (s < S)
        for (int r = ty; r < R; r += 4) sum += exp((double)ld_map(col + (size_t)r * S, rb) - (double)m);
    ss[ty][tx] = sum;
    __syncthreads();
    if (ty == 0 && s < S) {
        cmax[(size_t)h * S + s] = (double)m;
        csum[(size_t)h * S + s] = ((ss[0][tx] + ss[1][tx]) + ss[2][tx]) + ss[3][tx];
    }
}

// one row (h, r): p = softmax_S * softmax_R, then relu(p - v * median_S(p)) -> P[h][r][:]
__global__ __launch_bounds__(TB) void k_row_consensus(const float* maps, size_t pstride, int R, int S, int rb, const double* cmax,
                                                       const double* csum, float violence, float* P) {
    __shared__ SelShared sh;
    __shared__ RedShared red;
    __shared__ float line[MED_LDS];
    const int t = threadIdx.x, r = blockIdx.x, h = blockIdx.y;
    const float* xr = maps + (size_t)h * pstride + (size_t)r * S;
    float* pr = P + ((size_t)h * R + r) * S;
    const double* cm = cmax + (size_t)h * S;
    const double* cs = csum + (size_t)h * S;
    float m = -__builtin_inff();
    for (int s = t; s < S; s += TB) m = fmaxf(m, ld_map(xr + s, rb));
    m = block_max(m, red);
    double sum = 0.0;
    for (int s = t; s < S; s += TB) sum += exp((double)ld_map(xr + s, rb) - (double)m);
    sum = block_sum(sum, red);
    const bool in_lds = S <= MED_LDS;
    for (int s = t; s < S; s += TB) {
        const double x = (double)ld_map(xr + s, rb);
        const float p = (float)((exp(x - (double)m) / sum) * (exp(x - cm[s]) / cs[s]));
        pr[s] = p;
        if (in_lds) line[s] = p;
    }
    __syncthreads();
    const float med = in_lds ? block_median(line, 1, S, sh) : block_median(pr, 1, S, sh);
    const double sub = (double)violence * (double)med;
    for (int s = t; s < S; s += TB) {
        const float p = in_lds ? line[s] : pr[s];
        pr[s] = fmaxf((float)((double)p - sub), 0.f);
    }
}

// median over the rows of every column (h, s) of P
__global__ __launch_bounds__(TB) void k_col_median(const float* P, int R, int S, float* colmed) {
    __shared__ SelShared sh;
    __shared__ float line[MED_LDS];
    const int s = blockIdx.x, h = blockIdx.y;
    const float* v = P + (size_t)h * R * S + s;
    for (int r = threadIdx.x; r < R; r += TB) line[r] = v[(size_t)r * S];
    __syncthreads();
    const float med = block_median(line, 1, R, sh);
    if (threadIdx.x == 0) colmed[(size_t)h * S + s] = med;
}

// P <- relu(P - v * colmed)^2; energy = mean over heads; psum[r] = the row's sum over heads and frames
__global__ __launch_bounds__(TB) void k_sharpen(float* P, int H, int R, int S, const float* colmed, float violence, float* energy, double* psum) {
    __shared__ RedShared red;
    const int r = blockIdx.x;
    double acc = 0.0;
    for (int s = threadIdx.x; s < S; s += TB) {
        double e = 0.0;
        for (int h = 0; h < H; ++h) {
            float* p = P + ((size_t)h * R + r) * S + s;
            const float q = fmaxf((float)((double)*p - (double)violence * (double)colmed[(size_t)h * S + s]), 0.f);
            const float q2 = __fmul_rn(q, q);
            *p = q2;
            e += (double)q2;
        }
        energy[(size_t)r * S + s] = (float)(e / (double)H);
        acc += e;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) psum[r] = acc;
}

__device__ double total_of(const double* part, int R, RedShared& red) {
    double a = 0.0;
    for (int i = threadIdx.x; i < R; i += TB) a += part[i];
    return block_sum(a, red);
}

// psq[r] = the row's sum of (P - mean)^2
__global__ __launch_bounds__(TB) void k_dev_sq(const float* P, int H, int R, int S, const double* psum, double* psq) {
    __shared__ RedShared red;
    const int r = blockIdx.x;
    const double mean = total_of(psum, R, red) / ((double)H * (double)R * (double)S);
    double acc = 0.0;
    for (int h = 0; h < H; ++h) {
        const float* p = P + ((size_t)h * R + r) * S;
        for (int s = threadIdx.x; s < S; s += TB) {
            const double d = (double)p[s] - mean;
            acc += d * d;
        }
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) psq[r] = acc;
}

__device__ __forceinline__ int reflect(int i, int S) { return i < 0 ? -i : (i >= S ? 2 * (S - 1) - i : i); }

// the median of the w values f(reflect(s + k - w / 2)), k < w, w odd: the value with w / 2 values before it in (value, position) order
template <class F>
__device__ __forceinline__ float window_median(F f, int s, int S, int w) {
    if (w == 1) return f(s);
    const int half = w / 2;
    float med = 0.f;
    for (int a = 0; a < w; ++a) {
        const float va = f(reflect(s + a - half, S));
        int before = 0;
        for (int b = 0; b < w; ++b) {
            const float vb = f(reflect(s + b - half, S));
            before += (vb < va || (vb == va && b < a)) ? 1 : 0;
        }
        if (before == half) med = va;
    }
    return med;
}

// calc = mean over heads of medfilt_w((P - mean) / (std + 1e-9)).  The z-score is non-decreasing in P, so the window's median is taken
// on P and transformed once.
__global__ __launch_bounds__(TB) void k_zscore_calc(const float* P, int H, int R, int S, const double* psum, const double* psq, int w, float* calc) {
    __shared__ RedShared red;
    const int r = blockIdx.x;
    const double n = (double)H * (double)R * (double)S;
    const double mean = total_of(psum, R, red) / n;
    const double denom = sqrt(total_of(psq, R, red) / n) + 1e-9;
    for (int s = threadIdx.x; s < S; s += TB) {
        double acc = 0.0;
        for (int h = 0; h < H; ++h) {
            const float* p = P + ((size_t)h * R + r) * S;
            const float med = window_median([&](int i) { return p[i]; }, s, S, w);
            acc += (double)(float)(((double)med - mean) / denom);
        }
        calc[(size_t)r * S + s] = (float)(acc / (double)H);
    }
}

// ---------------------------------------------------------------------------------------------------------------- score matrix
// energy <- medfilt_w(mean over heads); pmin / pmax [r] = the row's extremes
__global__ __launch_bounds__(TB) void k_score_avg(const float* maps, size_t pstride, int H, int S, int rb, int w, float* energy, float* pmin, float* pmax) {
    __shared__ RedShared red;
    const int r = blockIdx.x;
    const float* xr = maps + (size_t)r * S;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    for (int s = threadIdx.x; s < S; s += TB) {
        const float e = window_median([&](int i) {
            double a = 0.0;
            for (int h = 0; h < H; ++h) a += (double)ld_map(xr + (size_t)h * pstride + i, rb);
            return (float)(a / (double)H);
        }, s, S, w);
        energy[(size_t)r * S + s] = e;
        mn = fminf(mn, e);
        mx = fmaxf(mx, e);
    }
    mn = block_min(mn, red);
    mx = block_max(mx, red);
    if (threadIdx.x == 0) { pmin[r] = mn; pmax[r] = mx; }
}

// energy <- (energy - min) / (max - min), or zeros when max - min <= 1e-9; calc = energy^2
__global__ __launch_bounds__(TB) void k_score_norm(int R, int S, const float* pmin, const float* pmax, float* energy, float* calc) {
    __shared__ RedShared red;
    const int r = blockIdx.x;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    for (int i = threadIdx.x; i < R; i += TB) { mn = fminf(mn, pmin[i]); mx = fmaxf(mx, pmax[i]); }
    mn = block_min(mn, red);
    mx = block_max(mx, red);
    const double range = (double)mx - (double)mn;
    for (int s = threadIdx.x; s < S; s += TB) {
        const size_t o = (size_t)r * S + s;
        const float e = range > 1e-9 ? (float)(((double)energy[o] - (double)mn) / range) : 0.f;
        energy[o] = e;
        calc[o] = __fmul_rn(e, e);
    }
}

// ---------------------------------------------------------------------------------------------------------------- DTW
// One workgroup per matrix.  Thread t owns the K consecutive rows i = t K + 1 .. t K + K (1-based, as the cost table's) and walks the
// anti-diagonals d = i + j.  Of the three predecessors of cell (i, j), cost[i][j-1] is the thread's own value of the previous diagonal,
// cost[i-1][j] is the row above's value of the previous diagonal (a register, or for the thread's first row the neighbour thread's last
// row through LDS), and cost[i-1][j-1] is the cost[i-1][j'] the same row read one diagonal earlier: two diagonals in registers, the
// third as the 1 K boundary values in LDS.  Inputs arrive 8 diagonals at a time (8 consecutive floats of each row) and the trace leaves
// as one 32-bit word per row and 16 diagonals (2 bits a cell), trace[d / 16][i - 1], so a sync never waits for a scattered byte store
// and the backtrace, which moves to row i or i - 1 and diagonal d - 1 or d - 2, mostly stays in the cache line it last read.
template <int K>
__global__ __launch_bounds__(1024) void k_dtw(const float* m, int R, int S, float sign, uint32_t* trace, int32_t* path, int32_t* path_len,
                                              int32_t* frames) {
    __shared__ float bnd[2][1024];
    const int b = blockIdx.x, t = threadIdx.x, nt = blockDim.x;
    const float INF = __builtin_inff();
    m += (size_t)b * R * S;
    const int G = (R + S) / 16 + 1;
    trace += (size_t)b * G * R;
    path += (size_t)b * 2 * (R + S);
    frames += (size_t)b * R * 2;
    float cur[K], c1s[K];
    uint32_t tw[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        cur[k] = INF;
        c1s[k] = (t * K + k == 0) ? 0.f : INF;
        tw[k] = 0u;
    }
    for (int r = t; r < R; r += nt) { frames[2 * r] = -1; frames[2 * r + 1] = -1; }
    bnd[0][t] = INF;
    bnd[1][t] = INF;
    __syncthreads();
    const int D = R + S;
    for (int d0 = 0; d0 <= D; d0 += 16) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            float xb[K][8];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int i = t * K + k + 1;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const int j = d0 + half * 8 + c - i;
                    xb[k][c] = (i <= R && j >= 1 && j <= S) ? __fmul_rn(sign, m[(size_t)(i - 1) * S + (j - 1)]) : 0.f;
                }
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int d = d0 + half * 8 + c;
                const float up = t > 0 ? bnd[(d + 1) & 1][t - 1] : INF;
#pragma unroll
                for (int k = K - 1; k >= 0; --k) {
                    const int i = t * K + k + 1, j = d - i;
                    if (i <= R && j >= 1 && j <= S) {
                        const float c1 = k > 0 ? cur[k > 0 ? k - 1 : 0] : up;
                        const float c0 = c1s[k], c2 = cur[k];
                        float cc;
                        uint32_t tt;
                        if (c0 < c1 && c0 < c2) { cc = c0; tt = 0u; }
                        else if (c1 < c0 && c1 < c2) { cc = c1; tt = 1u; }
                        else { cc = c2; tt = 2u; }
                        cur[k] = __fadd_rn(xb[k][c], cc);
                        c1s[k] = c1;
                        tw[k] |= tt << (2 * (half * 8 + c));
                    }
                }
                bnd[d & 1][t] = cur[K - 1];
                __syncthreads();
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int i = t * K + k + 1;
            if (i <= R) trace[(size_t)(d0 >> 4) * R + (i - 1)] = tw[k];
            tw[k] = 0u;
        }
    }
    __syncthreads();
    if (t != 0) return;
    // backtrace: the trace's row 0 reads "left" and its column 0 "up"
    int i = R, j = S, idx = R + S - 1, ci = -1, cg = -1, lastrow = -1;
    uint32_t w = 0u;
    while ((i > 0 || j > 0) && idx >= 0) {
        path[idx] = i - 1;
        path[D + idx] = j - 1;
        if (i >= 1) {
            if (i - 1 != lastrow) { frames[2 * (i - 1) + 1] = j - 1; lastrow = i - 1; }
            frames[2 * (i - 1)] = j - 1;
        }
        --idx;
        uint32_t tt;
        if (i == 0) tt = 2u;
        else if (j == 0) tt = 1u;
        else {
            const int d = i + j, g = d >> 4;
            if (g != cg || i != ci) { w = trace[(size_t)g * R + (i - 1)]; cg = g; ci = i; }
            tt = (w >> (2 * (d & 15))) & 3u;
        }
        if (tt == 0u) { --i; --j; }
        else if (tt == 1u) --i;
        else --j;
    }
    path_len[b] = R + S - 1 - idx;
}

// ---------------------------------------------------------------------------------------------------------------- score metrics
struct MonoShared {
    double first[TB], last[TB];
    int pairs[TB], ok[TB], sung[TB], covered[TB];
};

// per row: the maximum, and the centroid of the entries above time_weight (-1 without weight); a wave per row
__global__ __launch_bounds__(TB) void k_metric_rows(const float* energy, int R, int S, double time_weight, double* rows) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, r = blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    if (r >= R) return;
    const float* er = energy + ((size_t)b * R + r) * S;
    double mx = -__builtin_inf(), sw = 0.0, st = 0.0;
    for (int s = lane; s < S; s += 64) {
        const double e = (double)er[s];
        mx = fmax(mx, e);
        if (e > time_weight) { sw += e; st += e * (double)s; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        mx = fmax(mx, __shfl_down(mx, off, 64));
        sw += __shfl_down(sw, off, 64);
        st += __shfl_down(st, off, 64);
    }
    if (lane == 0) {
        rows[((size_t)b * R + r) * 2] = mx;
        rows[((size_t)b * R + r) * 2 + 1] = sw > 1e-9 ? st / sw : -1.0;
    }
}

__global__ __launch_bounds__(TB) void k_metrics(const float* energy, const int32_t* path, const int32_t* path_len, const int32_t* mask, int R,
                                                int S, double overlap, double inst_weight, const double* rows, double* out) {
    __shared__ RedShared red;
    __shared__ MonoShared ms;
    const int b = blockIdx.x, t = threadIdx.x;
    energy += (size_t)b * R * S;
    path += (size_t)b * 2 * (R + S);
    rows += (size_t)b * R * 2;
    // coverage and monotonicity: every thread summarises a run of rows, thread 0 joins the runs in order
    const int per = (R + TB - 1) / TB;
    int pairs = 0, ok = 0, sung = 0, covered = 0;
    double first = -1.0, last = -1.0;
    for (int r = t * per; r < min(R, (t + 1) * per); ++r) {
        if (mask[r] != 1) continue;
        ++sung;
        if (rows[2 * r] > 0.1) ++covered;
        const double c = rows[2 * r + 1];
        if (c < 0.0) continue;
        if (first < 0.0) first = c;
        else { ++pairs; if (c >= last - overlap) ++ok; }
        last = c;
    }
    ms.first[t] = first; ms.last[t] = last; ms.pairs[t] = pairs; ms.ok[t] = ok; ms.sung[t] = sung; ms.covered[t] = covered;
    // path confidence
    const int D = R + S, len = path_len[b];
    double te = 0.0, ts = 0.0;
    for (int p = D - len + t; p < D; p += TB) {
        const int pr = path[p], pc = path[D + p];
        if (pr < 0 || pc < 0) continue;
        const double wgt = mask[pr] == 0 ? inst_weight : 1.0;
        te += (double)energy[(size_t)pr * S + pc] * wgt;
        ts += wgt;
    }
    te = block_sum(te, red);
    ts = block_sum(ts, red);
    __syncthreads();
    if (t != 0) return;
    double prev = -1.0;
    pairs = ok = sung = covered = 0;
    for (int q = 0; q < TB; ++q) {
        sung += ms.sung[q];
        covered += ms.covered[q];
        pairs += ms.pairs[q];
        ok += ms.ok[q];
        if (ms.first[q] >= 0.0) {
            if (prev >= 0.0) { ++pairs; if (ms.first[q] >= prev - overlap) ++ok; }
            prev = ms.last[q];
        }
    }
    out[3 * b + 0] = sung > 0 ? (double)covered / (double)sung : 1.0;
    out[3 * b + 1] = pairs > 0 ? (double)ok / (double)pairs : 1.0;
    out[3 * b + 2] = (len > 0 && ts > 0.0) ? te / ts : 0.0;
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct MatrixWs {
    float* P;
    double *cmax, *csum, *psum, *psq;
    float *colmed, *pmin, *pmax;
    size_t bytes;
};
MatrixWs matrix_ws(void* ws, int H, int R, int S) {
    char* p = (char*)ws;
    size_t o = 0;
    MatrixWs m;
    m.P = (float*)(p + o); o += up256((size_t)H * R * S * 4);
    m.cmax = (double*)(p + o); o += up256((size_t)H * S * 8);
    m.csum = (double*)(p + o); o += up256((size_t)H * S * 8);
    m.psum = (double*)(p + o); o += up256((size_t)R * 8);
    m.psq = (double*)(p + o); o += up256((size_t)R * 8);
    m.colmed = (float*)(p + o); o += up256((size_t)H * S * 4);
    m.pmin = (float*)(p + o); o += up256((size_t)R * 4);
    m.pmax = (float*)(p + o); o += up256((size_t)R * 4);
    m.bytes = o;
    return m;
}
size_t dtw_ws_bytes(int R, int S, int batch) { return up256((size_t)batch * ((R + S) / 16 + 1) * R * 4); }
size_t metrics_ws_bytes(int R, int batch) { return up256((size_t)batch * R * 2 * 8); }

}  // namespace

size_t align_workspace_bytes(int H, int R, int S, int batch) {
    const size_t a = matrix_ws(nullptr, H, R, S).bytes, b = dtw_ws_bytes(R, S, batch), c = metrics_ws_bytes(R, batch);
    return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

int launch_align_median(const float* x, int outer, int n, int inner, float* out, hipStream_t st) {
    k_median<<<dim3(inner, outer), TB, 0, st>>>(x, n, inner, out);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_align_timestamp_matrix(const float* maps, size_t pstride, int H, int R, int S, float violence, int w, int rb, float* calc,
                                  float* energy, void* ws, hipStream_t st) {
    const MatrixWs m = matrix_ws(ws, H, R, S);
    k_col_stats<<<dim3((S + 63) / 64, H), dim3(64, 4), 0, st>>>(maps, pstride, R, S, rb, m.cmax, m.csum);
    ACE_LAUNCH_CHECK();
    k_row_consensus<<<dim3(R, H), TB, 0, st>>>(maps, pstride, R, S, rb, m.cmax, m.csum, violence, m.P);
    ACE_LAUNCH_CHECK();
    k_col_median<<<dim3(S, H), TB, 0, st>>>(m.P, R, S, m.colmed);
    ACE_LAUNCH_CHECK();
    k_sharpen<<<R, TB, 0, st>>>(m.P, H, R, S, m.colmed, violence, energy, m.psum);
    ACE_LAUNCH_CHECK();
    k_dev_sq<<<R, TB, 0, st>>>(m.P, H, R, S, m.psum, m.psq);
    ACE_LAUNCH_CHECK();
    k_zscore_calc<<<R, TB, 0, st>>>(m.P, H, R, S, m.psum, m.psq, S <= w / 2 ? 1 : w, calc);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_align_score_matrix(const float* maps, size_t pstride, int H, int R, int S, int w, int rb, float* calc, float* energy, void* ws,
                              hipStream_t st) {
    const MatrixWs m = matrix_ws(ws, H, R, S);
    k_score_avg<<<R, TB, 0, st>>>(maps, pstride, H, S, rb, S <= w / 2 ? 1 : w, energy, m.pmin, m.pmax);
    ACE_LAUNCH_CHECK();
    k_score_norm<<<R, TB, 0, st>>>(R, S, m.pmin, m.pmax, energy, calc);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_align_dtw(const float* mat, int batch, int R, int S, float sign, int32_t* path, int32_t* path_len, int32_t* frames, void* ws,
                     hipStream_t st) {
    uint32_t* trace = (uint32_t*)ws;
    const int K = R <= 1024 ? 1 : R <= 2048 ? 2 : R <= 4096 ? 4 : 8;
    const int nt = (((R + K - 1) / K) + 63) / 64 * 64;
    if (K == 1) k_dtw<1><<<batch, nt, 0, st>>>(mat, R, S, sign, trace, path, path_len, frames);
    else if (K == 2) k_dtw<2><<<batch, nt, 0, st>>>(mat, R, S, sign, trace, path, path_len, frames);
    else if (K == 4) k_dtw<4><<<batch, nt, 0, st>>>(mat, R, S, sign, trace, path, path_len, frames);
    else k_dtw<8><<<batch, nt, 0, st>>>(mat, R, S, sign, trace, path, path_len, frames);
    ACE_LAUNCH_CHECK();
    return 0;
}

int launch_align_score_metrics(const float* energy, const int32_t* path, const int32_t* path_len, const int32_t* mask, int batch, int R,
                               int S, double time_weight, double overlap, double inst_weight, double* out, void* ws, hipStream_t st) {
    k_metric_rows<<<dim3((R + TB / 64 - 1) / (TB / 64), batch), TB, 0, st>>>(energy, R, S, time_weight, (double*)ws);
    ACE_LAUNCH_CHECK();
    k_metrics<<<batch, TB, 0, st>>>(energy, path, path_len, mask, R, S, overlap, inst_weight, (const double*)ws, out);
    ACE_LAUNCH_CHECK();
    return 0;
}

}  // namespace ace355
