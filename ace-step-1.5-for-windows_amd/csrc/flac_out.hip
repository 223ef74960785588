// flac_out.hip - FLAC frames encoded on the GPU (the step after ace355_audio_interleave): the host encoder of
// audio_out.hip restated over 256 lanes per frame, byte for byte.  The per-frame rules live in flac_out.h (also run, serially, by
// tests/flac_out_host.cpp under the host sanitizers); the launches, grids and the scratch layout in flac_out_plan.h.
//
// Why the bytes are the host's: every decision is an integer sum or an integer comparison with the host's tie rule.  The sums are exact, so
// the order lanes and waves add in does not matter; shared words only ever take integer ADDs (LDS sums) or ORs (the bit buffer), which
// commute.  No global atomics.
#include <string>

#include "../../include/ace355.h"
#include "common.h"
#include "flac_out.h"
#include "flac_out_plan.h"

namespace ace355 {
namespace {

struct FlacOutArgs {
    const void* pcm;              // interleaved int16 [n_items][frames][channels], 4-byte aligned
    long long frames, blocks, units;
    int channels, sample_rate, n_items;
    uint8_t* slots;               // [units][FLAC_OUT_SLOT_BYTES]
    uint32_t* sizes;              // [units]
    long long* offsets;           // [units]
    uint8_t* out;
    long long item_stride;
    long long* records;           // [n_items][4]
};

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_xor_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}
// inclusive scan over the wave's 64 lanes
__device__ __forceinline__ uint32_t wave_scan_u32(uint32_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// The lanes of ONE wave searching one candidate's partition orders: LDS operations of a wave complete in order, so a compiler-level fence
// between the stores of one level and the loads of the next is all the lanes need.
struct WaveCtx {
    __device__ unsigned long long sum(unsigned long long v) const { return wave_sum_u64(v); }
    __device__ void sync() const {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
};

__global__ __launch_bounds__(FLAC_OUT_THREADS) void flac_out_frame_kernel(const FlacOutArgs a) {
    __shared__ FlacOutLds L;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long unit = blockIdx.x;
    if (unit >= a.units) return;
    const long long item = unit / a.blocks, blk = unit - item * a.blocks;
    const long long first = blk * FLAC_OUT_BLOCK;
    const int n = (int)(a.frames - first < FLAC_OUT_BLOCK ? a.frames - first : FLAC_OUT_BLOCK);
    const int channels = a.channels, ncand = channels == 2 ? 4 : 1, i0 = FLAC_OUT_PER_LANE * t;

    for (int w = t; w < FLAC_OUT_SLOT_WORDS; w += FLAC_OUT_THREADS) L.bits[w] = 0;
    for (int w = t; w < 4 * 2 * FLAC_OUT_MAX_PARTS; w += FLAC_OUT_THREADS) (&L.sums[0][0][0])[w] = 0;
    if (t < 20) (&L.tot[0][0])[t] = 0;
    if (t < 4) L.differs[t] = 0;
    if (channels == 2) {
        const uint32_t* src = static_cast<const uint32_t*>(a.pcm) + (item * a.frames + first);
        for (int i = t; i < n; i += FLAC_OUT_THREADS) L.pcm[flac_out_pcm_at(i)] = src[i];
    } else {
        const uint16_t* src = static_cast<const uint16_t*>(a.pcm) + (item * a.frames + first);
        for (int i = t; i < n; i += FLAC_OUT_THREADS) L.pcm[flac_out_pcm_at(i)] = src[i];
    }
    __syncthreads();

    // the candidates' totals
    int32_t s[FLAC_OUT_PER_LANE + 4];
    for (int c = 0; c < ncand; ++c) {
        flac_out_lane_signal(L.pcm, channels, c, i0, n, s);
        uint32_t tot[5], differs;
        flac_out_lane_stats(s, i0, n, flac_out_candidate(L.pcm[0], channels, c), tot, &differs);
#pragma unroll
        for (int o = 0; o < 5; ++o) tot[o] = wave_sum_u32(tot[o]);
        differs = wave_sum_u32(differs);
        if (lane == 0) {
#pragma unroll
            for (int o = 0; o < 5; ++o) atomicAdd(&L.tot[c][o], (unsigned long long)tot[o]);
            atomicAdd(&L.differs[c], differs);
        }
    }
    __syncthreads();

    // folded residuals of each candidate's order into its finest partitions
    for (int c = 0; c < ncand; ++c) {
        if (L.differs[c] == 0 || n <= 4) continue;
        uint64_t tot[5];
        for (int o = 0; o < 5; ++o) tot[o] = L.tot[c][o];
        const int order = flac_out_pick_order(tot), maxp = flac_out_max_porder(n, order);
        flac_out_lane_signal(L.pcm, channels, c, i0, n, s);
        unsigned long long* sums = L.sums[c][0];
        flac_out_lane_partition_sums(s, i0, n, order, n >> maxp, [sums](int p, uint64_t v) { atomicAdd(sums + p, (unsigned long long)v); });
    }
    __syncthreads();

    // wave c plans candidate c
    if (wave < ncand) {
        const int c = wave;
        const bool constant = L.differs[c] == 0;
        int order = 0, maxp = 0, porder = 0;
        uint64_t best = 0;
        if (!constant && n > 4) {
            uint64_t tot[5];
            for (int o = 0; o < 5; ++o) tot[o] = L.tot[c][o];
            order = flac_out_pick_order(tot), maxp = flac_out_max_porder(n, order);
            best = flac_out_partition_search(L.sums[c][0], L.sums[c][1], L.ks[c], L.sub[c].k, n, order, maxp, lane, 64, WaveCtx{}, &porder);
        }
        if (lane == 0) flac_out_finish_plan(&L.sub[c], n, c == 3 ? 17 : 16, constant, order, maxp, porder, best);
    }
    __syncthreads();

    int assign = 0, cand[2] = {0, 0};
    if (channels == 2) {
        const uint64_t b[4] = {L.sub[0].bits, L.sub[1].bits, L.sub[2].bits, L.sub[3].bits};
        assign = flac_out_pick_assignment(b, &cand[0], &cand[1]);
    }
    if (t == 0) {
        uint32_t* bits = L.bits;
        L.hdr_bytes = (uint32_t)flac_out_frame_header(n, assign, a.sample_rate, (uint64_t)blk,
                                                      [bits](int i, uint8_t v) { flac_out_put(bits, FLAC_OUT_SLOT_WORDS, 8u * (uint32_t)i, v, 8); });
    }

    // code lengths, their exclusive scan over the lanes
    uint32_t len[2] = {0, 0}, incl[2];
    for (int j = 0; j < channels; ++j) {
        flac_out_lane_signal(L.pcm, channels, cand[j], i0, n, s);
        len[j] = flac_out_lane_subframe<false>(s, i0, n, cand[j] == 3 ? 17 : 16, &L.sub[cand[j]], 0, nullptr, 0);
    }
    for (int j = 0; j < 2; ++j) {
        incl[j] = wave_scan_u32(len[j], lane);
        if (lane == 63) L.scan[j][wave] = incl[j];
    }
    __syncthreads();
    uint32_t base[2], total[2];
    for (int j = 0; j < 2; ++j) {
        uint32_t before = 0, all = 0;
        for (int w = 0; w < FLAC_OUT_WAVES; ++w) {
            const uint32_t v = L.scan[j][w];
            all += v;
            if (w < wave) before += v;
        }
        base[j] = before + incl[j] - len[j], total[j] = all;
    }
    const uint32_t hdr_bits = 8u * L.hdr_bytes;
    for (int j = 0; j < channels; ++j) {
        flac_out_lane_signal(L.pcm, channels, cand[j], i0, n, s);
        flac_out_lane_subframe<true>(s, i0, n, cand[j] == 3 ? 17 : 16, &L.sub[cand[j]], hdr_bits + (j ? total[0] : 0u) + base[j], L.bits, FLAC_OUT_SLOT_WORDS);
    }
    __syncthreads();

    // zero padding to a byte, CRC-16 from the lanes' chunk CRCs
    int body = (int)((hdr_bits + total[0] + total[1] + 7u) >> 3);
    if (body > FLAC_OUT_SLOT_BYTES - 2) body = FLAC_OUT_SLOT_BYTES - 2;   // (cannot happen: a frame never outgrows its verbatim form)
    const int chunk = 4 * ((((body + 3) >> 2) + FLAC_OUT_THREADS - 1) / FLAC_OUT_THREADS);
    const int b0 = t * chunk, b1 = b0 + chunk < body ? b0 + chunk : body;
    uint32_t crc = b0 < b1 ? flac_out_crc16_shift(flac_out_crc16_words(L.bits, b0, b1), (uint32_t)(body - b1)) : 0u;
    crc = wave_xor_u32(crc);
    if (lane == 0) L.crc[wave] = crc;
    __syncthreads();
    if (t == 0) {
        uint32_t c = 0;
        for (int w = 0; w < FLAC_OUT_WAVES; ++w) c ^= L.crc[w];
        flac_out_put(L.bits, FLAC_OUT_SLOT_WORDS, 8u * (uint32_t)body, c, 16);
    }
    __syncthreads();

    const int bytes = body + 2;
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.slots + unit * FLAC_OUT_SLOT_BYTES);
    for (int w = t; w < (bytes + 3) >> 2; w += FLAC_OUT_THREADS) dst[w] = __builtin_bswap32(L.bits[w]);
    if (t == 0) a.sizes[unit] = (uint32_t)bytes;
}

__global__ __launch_bounds__(FLAC_OUT_THREADS) void flac_out_offsets_kernel(const FlacOutArgs a) {
    __shared__ uint32_t part[4][FLAC_OUT_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long item = blockIdx.x;
    if (item >= a.n_items) return;
    long long carry = 0;
    uint32_t mn = 0xFFFFFFFFu, mx = 0, bad = 0;
    for (long long b0 = 0; b0 < a.blocks; b0 += FLAC_OUT_THREADS) {
        const long long b = b0 + t;
        const uint32_t sz = b < a.blocks ? a.sizes[item * a.blocks + b] : 0u;
        const uint32_t incl = wave_scan_u32(sz, lane);
        if (lane == 63) part[0][wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int w = 0; w < FLAC_OUT_WAVES; ++w) {
            all += part[0][w];
            if (w < wave) before += part[0][w];
        }
        if (b < a.blocks) {
            a.offsets[item * a.blocks + b] = carry + before + incl - sz;
            mn = sz < mn ? sz : mn, mx = sz > mx ? sz : mx, bad += sz < 8u || sz > (uint32_t)FLAC_OUT_SLOT_BYTES;
        }
        carry += all;
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t m1 = (uint32_t)__shfl_xor((int)mn, o, 64), m2 = (uint32_t)__shfl_xor((int)mx, o, 64);
        mn = m1 < mn ? m1 : mn, mx = m2 > mx ? m2 : mx;
    }
    bad = wave_sum_u32(bad);
    if (lane == 0) part[1][wave] = mn, part[2][wave] = mx, part[3][wave] = bad;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < FLAC_OUT_WAVES; ++w) {
            mn = part[1][w] < mn ? part[1][w] : mn, mx = part[2][w] > mx ? part[2][w] : mx, bad += part[3][w];
        }
        if (carry > a.item_stride - 42) ++bad;   // the gather leaves such frames out
        long long* r = a.records + FLAC_OUT_RECORD_INTS * item;
        r[0] = carry, r[1] = mn, r[2] = mx, r[3] = bad;
    }
}

__global__ __launch_bounds__(FLAC_OUT_THREADS) void flac_out_gather_kernel(const FlacOutArgs a) {
    const int t = threadIdx.x;
    const long long unit = blockIdx.x;
    if (unit >= a.units) return;
    const long long item = unit / a.blocks, off = a.offsets[unit];
    const uint32_t sz = a.sizes[unit];
    if (sz > (uint32_t)FLAC_OUT_SLOT_BYTES || off < 0 || off + (long long)sz > a.item_stride - 42) return;
    const int len = (int)sz;
    const uint8_t* src = a.slots + unit * FLAC_OUT_SLOT_BYTES;   // 16-byte aligned; the slot has room for a word past any frame
    uint8_t* dst = a.out + item * a.item_stride + 42 + off;
    int head = (int)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3);
    head = head < len ? head : len;
    if (t < head) dst[t] = src[t];
    const int nmid = (len - head) >> 2, sh = 8 * (head & 3);
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(src);
    uint32_t* dw = reinterpret_cast<uint32_t*>(dst + head);
    for (int w = t; w < nmid; w += FLAC_OUT_THREADS) {
        const uint32_t lo = sw[w + (head >> 2)];
        dw[w] = sh ? (lo >> sh) | (sw[w + (head >> 2) + 1] << (32 - sh)) : lo;
    }
    const int tail = head + 4 * nmid;
    if (tail + t < len) dst[tail + t] = src[tail + t];
}

int refuse(const char* what, const std::string& why) {
    set_error(std::string(what) + ": " + why);
    return ACE355_ERR_INVALID;
}

}  // namespace
}  // namespace ace355

using namespace ace355;

extern "C" {

int ace355_flac_out_plan(int32_t n_items, int64_t frames, int32_t channels, ace355_flac_out_plan_info* out) {
    ACE_CHECK(out, "flac_out_plan: null argument");
    const FlacOutPlan p = plan_flac_out(n_items, frames, channels);
    if (p.refusal) return refuse("flac_out_plan", p.refusal);
    out->blocks = p.blocks, out->units = p.units, out->frame_grid = p.frame_grid, out->offsets_grid = p.offsets_grid, out->gather_grid = p.gather_grid;
    out->item_stride = p.item_stride, out->sizes_at = p.sizes_at, out->offsets_at = p.offsets_at, out->scratch_bytes = p.scratch_bytes;
    out->out_bytes = p.out_bytes, out->records_bytes = p.records_bytes, out->launches = p.launches, out->frame_threads = p.frame_threads;
    out->offsets_threads = p.offsets_threads, out->gather_threads = p.gather_threads, out->frame_lds_bytes = p.frame_lds_bytes;
    out->offsets_lds_bytes = p.offsets_lds_bytes, out->slot_stride = p.slot_stride;
    return ACE355_OK;
}

int ace355_flac_out_encode(const int16_t* pcm_dev, int32_t n_items, int64_t frames, int32_t channels, int32_t sample_rate, void* scratch_dev,
                           int64_t scratch_bytes, void* out_dev, int64_t out_bytes, int64_t* records_dev, void* stream) {
    ACE_CHECK(pcm_dev && scratch_dev && out_dev && records_dev, "flac_out_encode: null argument");
    ACE_CHECK(sample_rate > 0 && sample_rate < (1 << 20), "flac_out_encode: sample rate outside STREAMINFO");
    const FlacOutPlan p = plan_flac_out(n_items, frames, channels);
    if (p.refusal) return refuse("flac_out_encode", p.refusal);
    ACE_CHECK(scratch_bytes >= p.scratch_bytes && out_bytes >= p.out_bytes, "flac_out_encode: the scratch or the output is smaller than the plan says");
    ACE_CHECK((reinterpret_cast<uintptr_t>(pcm_dev) & 3) == 0 && ((reinterpret_cast<uintptr_t>(scratch_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(records_dev) & 7) == 0,
              "flac_out_encode: the PCM must be 4-byte aligned, the scratch and the output 16-byte, the records 8-byte");
    FlacOutArgs a{};
    a.pcm = pcm_dev, a.frames = frames, a.blocks = p.blocks, a.units = p.units, a.channels = channels, a.sample_rate = sample_rate, a.n_items = n_items;
    char* sc = static_cast<char*>(scratch_dev);
    a.slots = reinterpret_cast<uint8_t*>(sc), a.sizes = reinterpret_cast<uint32_t*>(sc + p.sizes_at), a.offsets = reinterpret_cast<long long*>(sc + p.offsets_at);
    a.out = static_cast<uint8_t*>(out_dev), a.item_stride = p.item_stride, a.records = reinterpret_cast<long long*>(records_dev);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(flac_out_frame_kernel, dim3((unsigned)p.frame_grid), dim3(p.frame_threads), 0, s, a);
    ACE_LAUNCH_CHECK();
    hipLaunchKernelGGL(flac_out_offsets_kernel, dim3((unsigned)p.offsets_grid), dim3(p.offsets_threads), 0, s, a);
    ACE_LAUNCH_CHECK();
    hipLaunchKernelGGL(flac_out_gather_kernel, dim3((unsigned)p.gather_grid), dim3(p.gather_threads), 0, s, a);
    ACE_LAUNCH_CHECK();
    return ACE355_OK;
}

int ace355_flac_streaminfo(uint8_t* out42, int64_t frames, int32_t channels, int32_t sample_rate, uint32_t min_frame, uint32_t max_frame,
                           const uint8_t* md5_or_null) {
    ACE_CHECK(out42 && frames >= 0 && frames < FLAC_OUT_MAX_FRAMES && (channels == 1 || channels == 2) && sample_rate > 0 && sample_rate < (1 << 20) &&
                  min_frame < (1u << 24) && max_frame < (1u << 24),
              "flac_streaminfo: bad argument");
    flac_out_streaminfo(out42, frames, channels, sample_rate, min_frame, max_frame, md5_or_null);
    return ACE355_OK;
}

}  // extern "C"
