// lm_sample.hip - token selection on the 5 Hz LM's logits behind ace355.h: what LLMHandler's
// _apply_top_k_filter, _apply_top_p_filter and _sample_tokens (llm_inference.py:367-399) do to a [B, V] fp32 tensor, as one fixed chain of
// launches without a sort.
//
// Values are mapped to an order-preserving 32-bit key (zeros canonicalised, -inf lowest).  Both thresholds - the k-th largest value and
// the value at which the descending mass crosses p * Z - are found by radix selection over that key in three levels of 11 + 11 + 10 bits:
// a histogram launch over the row's chunks (counts for top-k; counts and fp64 masses for top-p), then a one-workgroup-per-row launch that
// adds the chunks' partials in chunk order and descends from the top bin.  A mask launch then writes the keep mask and the kept weights'
// per-chunk sums, and a last one-workgroup-per-row launch picks the token.  The cut of a row into chunks is lm_plan.h's plan_lm_pick, a
// function of V alone.
//
// Every hand-off is a launch boundary.  There is no floating-point atomic: a wave adds its lanes' masses per bin by a fixed lane pairing into a
// histogram of its own, the waves' histograms are added in wave order, the chunks' in chunk order.  Integer atomics (LDS counts, minima
// over thread indices) commute and cannot change a result.  All exponentials and sums are fp64.  A row's results depend on that row alone.
#include <math.h>

#include <string>

#include "../../include/ace355.h"
#include "common.h"
#include "lm_plan.h"

using namespace ace355;

namespace {

constexpr uint32_t KEY_NEGINF = 0x007FFFFFu;   // key_of(-inf): below every finite value's key
constexpr int HIST_BINS = 2048;                // bins of the widest level
constexpr int PER = LM_PICK_CHUNK / 256;       // ids of a chunk per thread
constexpr int GROUP = 8;                       // loads a thread has in flight: a chunk is walked as PER / GROUP groups of GROUP x 256 ids
static_assert(PER % GROUP == 0 && PER * 256 == LM_PICK_CHUNK, "a chunk is a whole number of groups");

__device__ __forceinline__ uint32_t key_of(float x) {
    uint32_t u = __float_as_uint(x);
    if ((u << 1) == 0) u = 0;   // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
__device__ __forceinline__ int level_shift(int l) { return l == 0 ? 21 : l == 1 ? 10 : 0; }
__device__ __forceinline__ int level_bins(int l) { return l < 2 ? 2048 : 1024; }

struct StatPart {   // one chunk of one row
    uint32_t maxkey;
    int first;      // lowest id of the chunk that holds maxkey
    int bad;        // a NaN or a +inf
    int finite;     // entries above -inf
};
struct RowStat {
    uint32_t maxkey;
    int first, bad;
};
struct MaskPart {
    double w;   // sum of the chunk's kept weights
    int kept, pad;
};
struct RowSel {   // the state of one radix selection of one row, written by sel_scan_kernel
    double carry;      // top-p: mass of the entries above the prefix group
    double target;     // top-p: p * Z
    uint32_t prefix;   // the key bits decided so far
    uint32_t rem;      // top-k: entries still to count inside the prefix group
    uint32_t key;      // after level 2: the threshold key
    uint32_t ties;     // top-p, after level 2: how many entries at the threshold value are kept, in ascending id
    int all;           // top-p: the mass never crosses p * Z: everything is kept
    int pad;
};

// The row's maximum, its first position and whether the row is bad, from the chunks' partials in chunk order: one thread fetches each
// partial (one memory latency instead of C), then every thread walks them in LDS.  sp: LM_PICK_MAX_CHUNKS entries; all threads call.
__device__ __forceinline__ RowStat row_stat(const StatPart* __restrict__ parts, int C, StatPart* sp) {
    for (int c = threadIdx.x; c < C; c += 256) sp[c] = parts[c];
    __syncthreads();
    RowStat r{0u, 0x7FFFFFFF, 0};
    int finite = 0;
    for (int c = 0; c < C; ++c) {
        const StatPart p = sp[c];
        if (p.maxkey > r.maxkey) { r.maxkey = p.maxkey; r.first = p.first; }
        r.bad |= p.bad;
        finite += p.finite;
    }
    r.bad |= finite == 0;
    return r;
}

// Sum of v over the wave, the same bits in every lane, in one fixed association: neighbours, pairs of neighbours, the two halves of a
// group of 8 and of a row of 16 (data-parallel lane moves: each lane adds the partner that holds the other half of its group, and
// addition commutes, so both get the same sum), then the four rows in row order.  About a seventh of the cost of the six cross-lane
// shuffles of wave_sum_d, which is what a histogram launch spends its time on.  Needs all 64 lanes active.
template <int CTRL>
__device__ __forceinline__ double lane_move_d(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double row_of(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
__device__ __forceinline__ double wave_sum_rows_d(double v) {
    v += lane_move_d<0xB1>(v);    // quad_perm [1, 0, 3, 2]
    v += lane_move_d<0x4E>(v);    // quad_perm [2, 3, 0, 1]
    v += lane_move_d<0x141>(v);   // row_half_mirror: lane i of a group of 8 reads lane 7 - i
    v += lane_move_d<0x140>(v);   // row_mirror: lane i of a row of 16 reads lane 15 - i
    return ((row_of(v, 0) + row_of(v, 16)) + row_of(v, 32)) + row_of(v, 48);
}

// Exclusive prefix of v over the 256 threads in thread order, in a fixed 16 x 16 association; *total = the sum of all.  s: 272 elements.
template <typename T>
__device__ __forceinline__ T excl_prefix_256(T v, T* s, T* total) {
    const int t = threadIdx.x;
    __syncthreads();
    s[t] = v;
    __syncthreads();
    if (t < 16) {
        T a = 0;
        for (int j = 0; j < 16; ++j) a += s[t * 16 + j];
        s[256 + t] = a;
    }
    __syncthreads();
    T e = 0, tot = 0;
    for (int g = 0; g < 16; ++g) {
        if (g < (t >> 4)) e += s[256 + g];
        tot += s[256 + g];
    }
    for (int j = t & ~15; j < t; ++j) e += s[j];
    *total = tot;
    return e;
}

// ------------------------------------------------------------------------------------------------ launch 1: maxima and bad entries
__global__ __launch_bounds__(256) void pick_stat_kernel(const float* __restrict__ logits, long stride, int V, int chunk, int C,
                                                        StatPart* __restrict__ parts) {
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int lo = c * chunk, hi = min(V, lo + chunk);
    const float* row = logits + (long)b * stride;
    uint32_t mk = 0;
    int first = 0x7FFFFFFF, bad = 0, fin = 0;
    for (int id = lo + tid; id < hi; id += 256) {
        const float x = row[id];
        bad |= (x != x) || (x == INFINITY);
        const uint32_t k = key_of(x);
        if (k > mk) { mk = k; first = id; }
        fin += k != KEY_NEGINF;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t ok = __shfl_xor(mk, o, 64);
        const int of = __shfl_xor(first, o, 64);
        if (ok > mk || (ok == mk && of < first)) { mk = ok; first = of; }
        bad |= __shfl_xor(bad, o, 64);
        fin += __shfl_xor(fin, o, 64);
    }
    __shared__ StatPart sp[4];
    if ((tid & 63) == 0) sp[tid >> 6] = StatPart{mk, first, bad, fin};
    __syncthreads();
    if (tid == 0) {
        StatPart r = sp[0];
        for (int w = 1; w < 4; ++w) {
            if (sp[w].maxkey > r.maxkey || (sp[w].maxkey == r.maxkey && sp[w].first < r.first)) { r.maxkey = sp[w].maxkey; r.first = sp[w].first; }
            r.bad |= sp[w].bad;
            r.finite += sp[w].finite;
        }
        parts[b * C + c] = r;
    }
}

// ------------------------------------------------------------------------------------------------ histogram of one level
// Entries of the chunk that lie in the selection's prefix group (level 0: all) and are not below `lo_sel`'s threshold (top-p runs over the
// survivors of top-k) are counted per bin, and with MASS their masses exp(x - max) are added per bin: per wave in lane order (one bin at a
// time: the lanes of the first unserved lane's bin are summed by wave_sum_rows_d and its leader adds the sum to the wave's own histogram),
// then the four waves in wave order.
template <bool MASS>
__global__ __launch_bounds__(256) void sel_hist_kernel(const float* __restrict__ logits, long stride, int V, int chunk, int C, int level,
                                                       const StatPart* __restrict__ stat, const RowSel* __restrict__ sel,
                                                       const RowSel* __restrict__ lo_sel, uint32_t* __restrict__ pcnt,
                                                       double* __restrict__ pmass) {
    __shared__ uint32_t cnt[HIST_BINS];
    __shared__ double wm[MASS ? 4 * HIST_BINS : 1];
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ StatPart stat_lds[LM_PICK_MAX_CHUNKS];
    const RowStat rs = row_stat(stat + b * C, C, stat_lds);
    if (rs.bad) return;
    if (MASS && level > 0 && sel[b].all) return;
    const int shift = level_shift(level), nb = level_bins(level);
    const uint32_t prefix = level > 0 ? sel[b].prefix : 0u;
    const uint32_t lo_key = lo_sel ? lo_sel[b].key : 0u;
    const double mx = (double)value_of(rs.maxkey);
    for (int i = tid; i < nb; i += 256) {
        cnt[i] = 0;
        if (MASS) {
            for (int w = 0; w < 4; ++w) wm[w * HIST_BINS + i] = 0.0;
        }
    }
    __syncthreads();
    const int lo = c * chunk, hi = min(V, lo + chunk);
    const float* row = logits + (long)b * stride;
    for (int base = lo; base < hi; base += GROUP * 256) {   // (uniform trip count: the ballots below need whole waves)
        float xs[GROUP];
#pragma unroll
        for (int g = 0; g < GROUP; ++g) {
            const int id = base + g * 256 + tid;
            xs[g] = id < hi ? row[id] : 0.f;
        }
#pragma unroll
        for (int g = 0; g < GROUP; ++g) {
            const int id = base + g * 256 + tid;
            const float x = xs[g];
            const uint32_t k = key_of(x);
            bool active = id < hi && k >= lo_key && (level == 0 || (k >> (shift + (level < 2 ? 11 : 10))) == prefix);
            if (MASS) active = active && k != KEY_NEGINF;
            const int bin = (int)((k >> shift) & (uint32_t)(nb - 1));
            if (active) atomicAdd(&cnt[bin], 1u);
            if (MASS) {
                unsigned long long todo = __ballot(active);
                if (todo) {
                    const double m = active ? exp((double)x - mx) : 0.0;
                    double* mine_hist = wm + wave * HIST_BINS;
                    while (todo) {
                        const int leader = __ffsll((long long)todo) - 1;
                        const int lb = __builtin_amdgcn_readlane(bin, leader);
                        const bool mine = active && bin == lb;
                        const unsigned long long mm = __ballot(mine);
                        const double s = wave_sum_rows_d(mine ? m : 0.0);
                        if (lane == leader) mine_hist[lb] += s;
                        todo &= ~mm;
                    }
                }
            }
        }
    }
    __syncthreads();
    const long out = (long)(b * C + c) * HIST_BINS;
    for (int i = tid; i < nb; i += 256) {
        pcnt[out + i] = cnt[i];
        if (MASS) pmass[out + i] = ((wm[i] + wm[HIST_BINS + i]) + wm[2 * HIST_BINS + i]) + wm[3 * HIST_BINS + i];
    }
}

// ------------------------------------------------------------------------------------------------ descent of one level
// One workgroup per row: the chunks' partial histograms are added in chunk order, thread t owns the 8 (4) bins below the top 8 t (4 t) in
// descending order, and the first bin at which the running count reaches `rem` (top-k) or the running mass exceeds p * Z (top-p) becomes
// the next piece of the prefix.  Level 2 leaves the threshold key, and for top-p how many of the entries AT that value are kept.
template <bool MASS>
__global__ __launch_bounds__(256) void sel_scan_kernel(int C, int level, int top_k, float top_p, const StatPart* __restrict__ stat,
                                                       RowSel* __restrict__ sel, const uint32_t* __restrict__ pcnt,
                                                       const double* __restrict__ pmass) {
    __shared__ uint32_t cnt[HIST_BINS];
    __shared__ double mass[MASS ? HIST_BINS : 1];
    __shared__ double sd[272];
    __shared__ uint32_t su[272];
    __shared__ int claim, lowest;
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ StatPart stat_lds[LM_PICK_MAX_CHUNKS];
    const RowStat rs = row_stat(stat + b * C, C, stat_lds);
    if (rs.bad) return;
    RowSel st = sel[b];
    if (level == 0) st = RowSel{0.0, 0.0, 0u, (uint32_t)top_k, 0u, 0xFFFFFFFFu, 0, 0};
    if (MASS && st.all) return;
    const int nb = level_bins(level), per = nb / 256, bits = level < 2 ? 11 : 10;
    {   // totals per bin, chunks added in chunk order; thread t takes bins t, t + 256, ..
        uint32_t n[HIST_BINS / 256] = {};
        double m[HIST_BINS / 256] = {};
#pragma unroll 8
        for (int c = 0; c < C; ++c) {
            const long at = (long)(b * C + c) * HIST_BINS + tid;
#pragma unroll
            for (int j = 0; j < HIST_BINS / 256; ++j) {
                if (j * 256 < nb) {
                    n[j] += pcnt[at + j * 256];
                    if (MASS) m[j] += pmass[at + j * 256];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < HIST_BINS / 256; ++j) {
            if (j * 256 < nb) {
                cnt[tid + j * 256] = n[j];
                if (MASS) mass[tid + j * 256] = m[j];
            }
        }
    }
    if (tid == 0) { claim = 256; lowest = -1; }
    __syncthreads();
    const int top = nb - 1 - tid * per;   // this thread's bins: top, top - 1, .., top - per + 1
    uint32_t ln = 0;
    double lm = 0.0;
    for (int j = 0; j < per; ++j) {
        ln += cnt[top - j];
        if (MASS) lm += mass[top - j];
    }
    if (!MASS) {
        uint32_t ntot;
        const uint32_t nex = excl_prefix_256<uint32_t>(ln, su, &ntot);
        // exactly one thread has nex < rem <= nex + ln (rem <= the group's count: k < V at level 0, by construction below it)
        if (nex < st.rem && nex + ln >= st.rem) {
            uint32_t cum = nex;
            for (int j = 0; j < per; ++j) {
                const uint32_t n = cnt[top - j];
                if (cum + n >= st.rem) {
                    st.prefix = (st.prefix << bits) | (uint32_t)(top - j);
                    st.rem -= cum;
                    if (level == 2) st.key = st.prefix;
                    sel[b] = st;
                    break;
                }
                cum += n;
            }
        }
        return;
    }
    double mtot;
    const double mex = excl_prefix_256<double>(lm, sd, &mtot);
    if (level == 0) { st.target = (double)top_p * mtot; st.carry = 0.0; }
    // the first occupied bin of this thread's walk at which the running mass exceeds the target; a thread that starts beyond the target
    // claims its first occupied bin (an ulp between two associations of the same sum must not lose the crossing); the lowest thread wins
    int my_bin = -1;
    double my_before = 0.0, cum = st.carry + mex;
    int low_bin = -1;
    double low_before = 0.0;
    for (int j = 0; j < per; ++j) {
        const double nxt = cum + mass[top - j];
        if (my_bin < 0 && nxt > st.target && cnt[top - j]) { my_bin = top - j; my_before = cum; }
        if (cnt[top - j]) { low_bin = top - j; low_before = cum; }
        cum = nxt;
    }
    if (my_bin >= 0) atomicMin(&claim, tid);
    if (low_bin >= 0) atomicMax(&lowest, tid);
    __syncthreads();
    int bin;
    double before;
    if (claim < 256) {
        if (tid != claim) return;
        bin = my_bin; before = my_before;
    } else if (level == 0 || lowest < 0) {   // the whole mass stays within p * Z: everything is kept
        if (tid == 0) { st.all = 1; st.key = 0u; st.ties = 0xFFFFFFFFu; sel[b] = st; }
        return;
    } else {   // below level 0 the group is known to cross: its lowest value takes the crossing
        if (tid != lowest) return;
        bin = low_bin; before = low_before;
    }
    st.prefix = (st.prefix << bits) | (uint32_t)bin;
    st.carry = before;
    if (level == 2) {
        st.key = st.prefix;
        // entries at the threshold value, in ascending id: the r-th (r = 0 ..) is kept iff before + r * m <= target
        const uint32_t n = cnt[bin];
        const double m = exp((double)value_of(st.key) - (double)value_of(rs.maxkey));
        uint32_t r = n;
        if (m > 0.0 && n > 0) {
            const double q = (st.target - before) / m;
            r = q < 0.0 ? 1u : q >= (double)n ? n : (uint32_t)q + 1u;
            while (r < n && before + (double)r * m <= st.target) ++r;
            while (r > 1 && before + (double)(r - 1) * m > st.target) --r;
        }
        st.ties = r < 1 ? 1u : r;
    }
    sel[b] = st;
}

// ------------------------------------------------------------------------------------------------ mask and weights
// keep = finite, not below the top-k threshold, above the top-p threshold or among its first `ties` entries in ascending id (the ranks of
// a chunk start at the count of threshold entries in the chunks before it: level 2's partial counts).  The chunk's kept weights
// exp((x - max) / T) are added per thread in id order, then by the xor tree, then over the waves in order.
__global__ __launch_bounds__(256) void pick_mask_kernel(const float* __restrict__ logits, long stride, int V, int chunk, int C, int k_on,
                                                        int p_on, float temperature, const StatPart* __restrict__ stat,
                                                        const RowSel* __restrict__ sel_k, const RowSel* __restrict__ sel_p,
                                                        const uint32_t* __restrict__ pcnt, uint8_t* __restrict__ keep, MaskPart* __restrict__ parts) {
    __shared__ uint32_t wcnt[4];
    __shared__ double wsum[4];
    __shared__ int wkept[4];
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lo = c * chunk, hi = min(V, lo + chunk);
    __shared__ StatPart stat_lds[LM_PICK_MAX_CHUNKS];
    const RowStat rs = row_stat(stat + b * C, C, stat_lds);
    uint8_t* krow = keep + (long)b * V;
    if (rs.bad) {
        for (int id = lo + tid; id < hi; id += 256) krow[id] = 0;
        if (tid == 0) parts[b * C + c] = MaskPart{0.0, 0, 0};
        return;
    }
    const uint32_t tk = k_on ? sel_k[b].key : 0u;
    const bool ranked = p_on && !sel_p[b].all;
    const uint32_t tp = ranked ? sel_p[b].key : 0u, ties = ranked ? sel_p[b].ties : 0xFFFFFFFFu;
    __shared__ uint32_t before;   // threshold entries in the chunks before this one (integer adds commute)
    if (tid == 0) before = 0;
    __syncthreads();
    if (ranked) {
        const uint32_t bin = tp & 1023u;
        for (int cc = tid; cc < c; cc += 256) atomicAdd(&before, pcnt[(long)(b * C + cc) * HIST_BINS + bin]);
    }
    __syncthreads();
    uint32_t rank0 = before;
    const double mx = (double)value_of(rs.maxkey), T = (double)temperature;
    const float* row = logits + (long)b * stride;
    double w = 0.0;
    int kept = 0;
    for (int base = lo; base < hi; base += GROUP * 256) {
        float xs[GROUP];
#pragma unroll
        for (int g = 0; g < GROUP; ++g) {
            const int id = base + g * 256 + tid;
            xs[g] = id < hi ? row[id] : 0.f;
        }
#pragma unroll
        for (int g = 0; g < GROUP; ++g) {
            const int id = base + g * 256 + tid;
            const float x = xs[g];
            const uint32_t k = key_of(x);
            bool ok = id < hi && k != KEY_NEGINF && k >= tk && k >= tp;
            if (ranked) {   // (uniform over the workgroup)
                const bool tie = ok && k == tp;
                const unsigned long long tb = __ballot(tie);
                if (lane == 0) wcnt[wave] = (uint32_t)__popcll(tb);
                __syncthreads();
                uint32_t r = rank0 + (uint32_t)__popcll(tb & ((1ull << lane) - 1ull)), all = 0;
                for (int wv = 0; wv < 4; ++wv) {
                    if (wv < wave) r += wcnt[wv];
                    all += wcnt[wv];
                }
                if (tie && r >= ties) ok = false;
                rank0 += all;
                __syncthreads();
            }
            if (id < hi) {
                krow[id] = ok ? 1 : 0;
                if (ok) {
                    ++kept;
                    if (temperature > 0.f) w += exp(((double)x - mx) / T);
                }
            }
        }
    }
    w = wave_sum_d(w);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o, 64);
    if (lane == 0) { wsum[wave] = w; wkept[wave] = kept; }
    __syncthreads();
    if (tid == 0) parts[b * C + c] = MaskPart{((wsum[0] + wsum[1]) + wsum[2]) + wsum[3], wkept[0] + wkept[1] + wkept[2] + wkept[3], 0};
}

// ------------------------------------------------------------------------------------------------ the token
// One workgroup per row.  Greedy: the first position of the row's maximum (launch 1 has it).  Sampling: the chunks' weight sums in chunk
// order give W and the chunk in which the running sum exceeds u * W; inside it thread t walks the kept weights of its PER consecutive ids
// behind the threads before it, and the first id whose running sum exceeds the rest of the target is the token; if rounding lets none
// exceed it, the last kept id with a non-zero weight.
__global__ __launch_bounds__(256) void pick_token_kernel(const float* __restrict__ logits, long stride, int V, int chunk, int C, int masked,
                                                         float temperature, const float* __restrict__ u, const StatPart* __restrict__ stat,
                                                         const uint8_t* __restrict__ keep, const MaskPart* __restrict__ parts,
                                                         int64_t* __restrict__ tokens, int32_t* __restrict__ kept_out) {
    __shared__ double sd[272];
    __shared__ int found, last, s_chunk;
    __shared__ double s_rest;
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ StatPart stat_lds[LM_PICK_MAX_CHUNKS];
    const RowStat rs = row_stat(stat + b * C, C, stat_lds);
    if (rs.bad) {
        if (tid == 0) { tokens[b] = -1; if (kept_out) kept_out[b] = 0; }
        return;
    }
    __shared__ MaskPart mp[LM_PICK_MAX_CHUNKS];
    if (masked) {
        for (int c = tid; c < C; c += 256) mp[c] = parts[b * C + c];
    }
    __syncthreads();
    if (masked && kept_out && tid == 0) {
        int n = 0;
        for (int c = 0; c < C; ++c) n += mp[c].kept;
        kept_out[b] = n;
    }
    if (!(temperature > 0.f)) {
        if (tid == 0) tokens[b] = rs.first;
        return;
    }
    if (tid == 0) {
        double W = 0.0;
        for (int c = 0; c < C; ++c) W += mp[c].w;
        const double target = (double)u[b] * W;
        int pick = -1, lastc = 0;
        double cum = 0.0, before = 0.0;
        for (int c = 0; c < C; ++c) {
            const double wc = mp[c].w;
            if (wc > 0.0) lastc = c;
            if (pick < 0 && cum + wc > target) { pick = c; before = cum; }
            cum += wc;
        }
        s_chunk = pick >= 0 ? pick : lastc;
        s_rest = pick >= 0 ? target - before : INFINITY;
        found = 0x7FFFFFFF;
        last = -1;
    }
    __syncthreads();
    const int c = s_chunk, lo = c * chunk, hi = min(V, lo + chunk);
    const double rest = s_rest, mx = (double)value_of(rs.maxkey), T = (double)temperature;
    const float* row = logits + (long)b * stride;
    const uint8_t* krow = keep + (long)b * V;
    // thread t owns the PER consecutive ids from lo + PER t: its weights in id order, the threads' sums by the fixed prefix
    double w[PER], mine = 0.0;
    const int id0 = lo + tid * PER;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int id = id0 + i;
        w[i] = 0.0;
        if (id < hi && krow[id]) w[i] = exp(((double)row[id] - mx) / T);
        mine += w[i];
    }
    double tot;
    double run = excl_prefix_256<double>(mine, sd, &tot);
    int hit = 0x7FFFFFFF, tail = -1;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        run += w[i];
        if (w[i] > 0.0) {
            tail = id0 + i;
            if (hit == 0x7FFFFFFF && run > rest) hit = id0 + i;
        }
    }
    if (hit != 0x7FFFFFFF) atomicMin(&found, hit);   // (a thread that starts beyond the target claims its first weighted id; the lowest id wins)
    if (tail >= 0) atomicMax(&last, tail);
    __syncthreads();
    if (tid == 0) tokens[b] = found != 0x7FFFFFFF ? found : last;
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

struct PickWorkspace {
    size_t stat, sel, parts, pcnt, pmass, keep, total;
};
PickWorkspace pick_workspace(int B, int V) {
    PickWorkspace w{};
    const LmPickPlan p = plan_lm_pick(V);
    if (B < 1 || B > LM_MAX_SEQS || p.chunks == 0) return w;
    const size_t rows = (size_t)B * p.chunks;
    size_t at = 0;
    w.stat = at; at += align256(rows * sizeof(StatPart));
    w.sel = at; at += align256((size_t)2 * B * sizeof(RowSel));
    w.parts = at; at += align256(rows * sizeof(MaskPart));
    w.pcnt = at; at += align256(rows * HIST_BINS * sizeof(uint32_t));
    w.pmass = at; at += align256(rows * HIST_BINS * sizeof(double));
    w.keep = at; at += align256((size_t)B * V);
    w.total = at;
    return w;
}

int refuse(const std::string& msg) {
    set_error("lm_pick: " + msg);
    return ACE355_ERR_INVALID;
}

}  // namespace

extern "C" {

size_t ace355_lm_pick_workspace_bytes(int B, int V) { return pick_workspace(B, V).total; }

int ace355_lm_pick_plan(int V, int32_t* chunk_out, int32_t* chunks_out) {
    const LmPickPlan p = plan_lm_pick(V);
    ACE_CHECK(p.chunks > 0 && chunk_out && chunks_out, "lm_pick_plan: V must be 1 .. 1048576");
    *chunk_out = p.chunk;
    *chunks_out = p.chunks;
    return ACE355_OK;
}

int ace355_lm_pick(const float* logits_dev, int64_t row_stride, int B, int V, const ace355_lm_pick_params* p, const float* u_dev,
                   int64_t* tokens_dev, int32_t* kept_dev, uint8_t* keep_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (B < 1 || B > ACE355_LM_MAX_SEQS) return refuse("B must be 1 .. " + std::to_string(ACE355_LM_MAX_SEQS));
    if (V < 1 || V > LM_PICK_MAX_V) return refuse("V must be 1 .. " + std::to_string(LM_PICK_MAX_V));
    if (row_stride < V) return refuse("row_stride is smaller than V");
    if (!logits_dev || !p || !tokens_dev || !workspace_dev) return refuse("logits, params, tokens and workspace must not be null");
    if (p->temperature > 0.f && !u_dev) return refuse("u is required when temperature > 0");
    if (p->temperature != p->temperature || p->top_p != p->top_p) return refuse("top_p and temperature must not be NaN");
    const PickWorkspace ws = pick_workspace(B, V);
    if (workspace_bytes < ws.total) return refuse("workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(ws.total) + " needed");
    if ((uintptr_t)workspace_dev & 7) return refuse("workspace must be 8-byte aligned");

    const LmPickPlan plan = plan_lm_pick(V);
    const int C = plan.chunks, chunk = plan.chunk;
    char* base = (char*)workspace_dev;
    StatPart* stat = (StatPart*)(base + ws.stat);
    RowSel* sel_k = (RowSel*)(base + ws.sel);
    RowSel* sel_p = sel_k + B;
    MaskPart* parts = (MaskPart*)(base + ws.parts);
    uint32_t* pcnt = (uint32_t*)(base + ws.pcnt);
    double* pmass = (double*)(base + ws.pmass);
    uint8_t* keep = keep_dev ? keep_dev : (uint8_t*)(base + ws.keep);
    hipStream_t s = (hipStream_t)stream;
    const bool k_on = p->top_k > 0 && p->top_k < V, p_on = p->top_p > 0.f && p->top_p < 1.f, sample = p->temperature > 0.f;
    const bool masked = sample || kept_dev || keep_dev;   // greedy with no mask asked for needs no threshold: the maximum always survives
    const dim3 grid(C, B);

    pick_stat_kernel<<<grid, 256, 0, s>>>(logits_dev, row_stride, V, chunk, C, stat);
    ACE_LAUNCH_CHECK();
    if (masked) {
        if (k_on) {   // (with top-k off, the default, its three levels are not launched)
            for (int level = 0; level < 3; ++level) {
                sel_hist_kernel<false><<<grid, 256, 0, s>>>(logits_dev, row_stride, V, chunk, C, level, stat, sel_k, nullptr, pcnt, nullptr);
                ACE_LAUNCH_CHECK();
                sel_scan_kernel<false><<<B, 256, 0, s>>>(C, level, p->top_k, 0.f, stat, sel_k, pcnt, nullptr);
                ACE_LAUNCH_CHECK();
            }
        }
        if (p_on) {
            for (int level = 0; level < 3; ++level) {
                sel_hist_kernel<true><<<grid, 256, 0, s>>>(logits_dev, row_stride, V, chunk, C, level, stat, sel_p, k_on ? sel_k : nullptr, pcnt, pmass);
                ACE_LAUNCH_CHECK();
                sel_scan_kernel<true><<<B, 256, 0, s>>>(C, level, 0, p->top_p, stat, sel_p, pcnt, pmass);
                ACE_LAUNCH_CHECK();
            }
        }
        pick_mask_kernel<<<grid, 256, 0, s>>>(logits_dev, row_stride, V, chunk, C, k_on, p_on, p->temperature, stat, sel_k, sel_p, pcnt, keep, parts);
        ACE_LAUNCH_CHECK();
    }
    pick_token_kernel<<<B, 256, 0, s>>>(logits_dev, row_stride, V, chunk, C, masked, p->temperature, u_dev, stat, keep, parts, tokens_dev, kept_dev);
    ACE_LAUNCH_CHECK();
    return ACE355_OK;
}

}  // extern "C"
