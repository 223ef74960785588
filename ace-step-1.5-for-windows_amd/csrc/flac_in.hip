// flac_in.hip - FLAC (RFC 9639) frames decoded on the GPU into the PCM payload ace355_audio_in_run reads: 16 to 24 bits per sample, 1 or
// 2 channels, every subframe form.  The file's bytes go up as they are; the host only walks the frame headers (ace355_flac_index) and
// the launches are the ones flac_in_plan.h names.  The per-frame routines live in flac_in.h, which the host test program compiles too.
//
// Cost model.  A FLAC frame is a serial bitstream: the second subframe starts where the first ends, and every Rice code starts where the
// previous one ends.  So the unit of parallel work is the frame, and a lane costs
//   entropy   channels x block residuals: per residual one count-leading-zeros on a 64-bit window, a k-bit field, a zig-zag and one
//             4-byte store; one dword load per 32 bits of stream (about every 2-3 residuals), which is the latency that bounds a lane;
//             then the CRC-16, one table step per byte of the frame (4 bytes per dword load);
//   restore   block x order multiply-adds (int64 sums for LPC), the history read back from the lane's own scratch row;
//   finish    one sample: two loads, shifts and adds, one store - the only pass with coalesced traffic.
// Lanes of a wave follow different bitstreams: loads are byte-granular and fully divergent, and a wave is as slow as its slowest lane
// whether 1 or 64 lanes are live.  The chip has 1024 SIMDs, so the plan gives every frame a wave of its own until there are more than
// 1024 frames.  A 30 s clip at 4096-sample blocks is 323 frames: 323 single-lane waves, a third of the SIMDs busy, and the pass takes
// as long as one frame takes.  A 240 s clip is 2584 frames: 3 live lanes per wave, 862 waves, still one frame's latency times a small
// factor.  Neither comes near the chip's bandwidth: the passes are latency bound by construction, and the time is flat in the clip
// length until frames / 1024 lanes per wave fill the waves (about 65 000 frames, 100 minutes of audio).
// The scratch is [channel][sample]: entropy and restore lanes walk their own rows (stride = a block between lanes, no sharing of cache
// lines to gain), the finish pass reads both rows and writes the interleaved output with consecutive lanes on consecutive samples.
// No atomics of any kind: the status reduction is one workgroup's min over (frame << 3 | code).
#include <string.h>

#include <string>

#include "../../include/ace355.h"
#include "common.h"
#include "flac_in.h"
#include "flac_in_plan.h"

static_assert(sizeof(ace355::FlacSubDesc) == 4 * ace355::FLAC_DESC_INTS && ace355::FLAC_DESC_INTS == ace355::FLAC_IN_DESC_INTS, "descriptor size");
static_assert(ACE355_FLAC_OK == ace355::FLAC_OK && ACE355_FLAC_HEADER_MISMATCH == ace355::FLAC_HEADER_MISMATCH &&
              ACE355_FLAC_RESERVED == ace355::FLAC_RESERVED && ACE355_FLAC_OVERRUN == ace355::FLAC_OVERRUN &&
              ACE355_FLAC_SAMPLE_COUNT == ace355::FLAC_SAMPLE_COUNT && ACE355_FLAC_CRC16 == ace355::FLAC_CRC16, "status codes");

namespace ace355 {
namespace {

struct FlacInArgs {
    const uint8_t* file;        // 4-byte aligned, readable up to the next multiple of 4 past file_bytes
    long long file_bytes;
    const int64_t* table;       // [frames][4]: byte offset, byte length, first sample, block size
    long long frames, total;
    int32_t* resid;             // [channels][total]
    FlacSubDesc* desc;          // [frames][2]
    int32_t* frame_words;       // [frames][2]: status, channel assignment
    void* out;
    int32_t* status_out;        // [2]: first bad frame (-1: none), its code
    FlacStreamParams sp;
    int max_block, lanes, tiles;
};

struct FlacRow {
    long long offset, bytes, first, block;
    bool ok;
};

// A row the kernels may act on: its bytes inside the file, its samples inside the stream, its block within the plan's bound.
__device__ __forceinline__ FlacRow load_row(const FlacInArgs& a, long long f) {
    FlacRow r;
    r.offset = a.table[4 * f], r.bytes = a.table[4 * f + 1], r.first = a.table[4 * f + 2], r.block = a.table[4 * f + 3];
    r.ok = r.offset >= 0 && r.bytes >= 0 && r.offset <= a.file_bytes && r.bytes <= a.file_bytes - r.offset && r.block >= 1 &&
           r.block <= a.max_block && r.first >= 0 && r.first <= a.total && r.block <= a.total - r.first;
    return r;
}

__global__ __launch_bounds__(FLAC_IN_WAVE) void flac_entropy_kernel(const FlacInArgs a) {
    if ((int)threadIdx.x >= a.lanes) return;
    const long long f = (long long)blockIdx.x * a.lanes + threadIdx.x;
    if (f >= a.frames) return;
    const FlacRow r = load_row(a, f);
    int32_t assign = 0;
    int st = FLAC_HEADER_MISMATCH;
    if (r.ok)
        st = flac_frame_entropy(a.file, r.offset, r.bytes, a.sp.variable ? (uint64_t)r.first : (uint64_t)f, (int)r.block, a.sp, a.resid + r.first,
                                a.resid + a.total * (a.sp.channels - 1) + r.first, a.desc + 2 * f, &assign);
    a.frame_words[2 * f] = st, a.frame_words[2 * f + 1] = assign;
}

__global__ __launch_bounds__(FLAC_IN_WAVE) void flac_restore_kernel(const FlacInArgs a) {
    if ((int)threadIdx.x >= a.lanes) return;
    const long long u = (long long)blockIdx.x * a.lanes + threadIdx.x;
    const long long f = u / a.sp.channels;
    const int c = (int)(u - f * a.sp.channels);
    if (f >= a.frames || a.frame_words[2 * f] != FLAC_OK) return;
    const FlacRow r = load_row(a, f);
    if (!r.ok) return;
    flac_subframe_restore(a.resid + a.total * c + r.first, (int)r.block, a.desc + 2 * f + c);
}

__global__ __launch_bounds__(FLAC_IN_FINISH_THREADS) void flac_finish_kernel(const FlacInArgs a) {
    const long long f = blockIdx.x / a.tiles;
    const int i = (int)(blockIdx.x - f * a.tiles) * FLAC_IN_FINISH_THREADS + threadIdx.x;
    const FlacRow r = load_row(a, f);
    if (!r.ok || i >= r.block) return;
    const bool good = a.frame_words[2 * f] == FLAC_OK;   // a frame that failed leaves zeros
    const int assign = a.frame_words[2 * f + 1];
    const long long at = r.first + i;
    int32_t l = 0, rr = 0;
    if (good) {
        const int32_t a0 = a.resid[at], a1 = a.sp.channels == 2 ? a.resid[a.total + at] : 0;
        flac_finish_sample(a0, a1, a.desc[2 * f].wasted, a.sp.channels == 2 ? a.desc[2 * f + 1].wasted : 0, a.sp.channels == 2 ? assign : 0, &l, &rr);
    }
    if (a.sp.bps == 16) {
        if (a.sp.channels == 2) static_cast<uint32_t*>(a.out)[at] = ((uint32_t)l & 0xffffu) | ((uint32_t)rr << 16);
        else static_cast<int16_t*>(a.out)[at] = (int16_t)l;
    } else {
        const int up = 32 - a.sp.bps;
        int32_t* o = static_cast<int32_t*>(a.out);
        if (a.sp.channels == 2) {
            o[2 * at] = (int32_t)((uint32_t)l << up), o[2 * at + 1] = (int32_t)((uint32_t)rr << up);
        } else o[at] = (int32_t)((uint32_t)l << up);
    }
}

__global__ __launch_bounds__(FLAC_IN_STATUS_THREADS) void flac_status_kernel(const FlacInArgs a) {
    __shared__ unsigned long long best[FLAC_IN_STATUS_THREADS];
    unsigned long long m = ~0ull;
    for (long long f = threadIdx.x; f < a.frames; f += FLAC_IN_STATUS_THREADS) {
        const int st = a.frame_words[2 * f];
        if (st != FLAC_OK && m == ~0ull) m = ((unsigned long long)f << 3) | (unsigned)(st & 7);   // (f ascends: the first one stays)
    }
    best[threadIdx.x] = m;
    __syncthreads();
    for (int s = FLAC_IN_STATUS_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && best[threadIdx.x + s] < best[threadIdx.x]) best[threadIdx.x] = best[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long b = best[0];
        a.status_out[0] = b == ~0ull ? -1 : (int32_t)(b >> 3);
        a.status_out[1] = b == ~0ull ? FLAC_OK : (int32_t)(b & 7);
    }
}

int refuse(const char* what, const std::string& why) {
    set_error(std::string(what) + ": " + why);
    return ACE355_ERR_INVALID;
}

}  // namespace
}  // namespace ace355

using namespace ace355;

extern "C" {

int ace355_flac_index(const uint8_t* data, int64_t size, ace355_flac_stream_info* info, int64_t* table, int64_t capacity, int64_t* n_frames) {
    ACE_CHECK(data && size > 0 && info && n_frames && capacity >= 0 && (table || capacity == 0), "flac_index: bad argument");
    FlacInfo fi;
    if (const char* e = flac_parse_header(data, (size_t)size, &fi)) return refuse("flac_index", e);
    info->total_samples = fi.frames, info->first_frame = (int64_t)fi.first_frame, info->channels = fi.channels, info->bits_per_sample = fi.bps;
    info->sample_rate = fi.sample_rate, info->min_block = fi.min_block, info->max_block = fi.max_block, info->variable_blocks = 0;
    *n_frames = 0;
    if (fi.bps < 16 || fi.bps > 24) return refuse("flac_index", std::to_string(fi.bps) + " bits per sample (the GPU decode takes 16 .. 24)");
    if (fi.channels > 2) return refuse("flac_index", std::to_string(fi.channels) + " channels (the GPU decode takes 1 or 2)");
    if (fi.max_block > FLAC_IN_MAX_BLOCK || fi.max_block < FLAC_IN_MIN_BLOCK)
        return refuse("flac_index", "STREAMINFO max block " + std::to_string(fi.max_block) + " (the GPU decode takes 16 .. 16384)");
    if (fi.frames == 0) return refuse("flac_index", "STREAMINFO does not say how many samples the stream holds");
    const FlacStreamParams sp0{fi.channels, fi.bps, fi.sample_rate, 0};
    auto candidate = [&](int64_t at, int variable, uint64_t number, FlacFrameHeader* h) {
        if (flac_parse_frame_header(data + at, size - at, h) != FLAC_OK) return false;
        return h->variable == variable && h->number == number && h->channels == sp0.channels && h->block <= fi.max_block &&
               (h->sample_rate == 0 || h->sample_rate == sp0.sample_rate) && (h->bps == 0 || h->bps == sp0.bps);
    };
    int64_t pos = (int64_t)fi.first_frame, done = 0, count = 0;
    if (pos + 2 > size || data[pos] != 0xFF || (data[pos + 1] & 0xFE) != 0xF8) return refuse("flac_index", "no frame sync where the metadata ends");
    const int variable = data[pos + 1] & 1;
    info->variable_blocks = variable;
    FlacFrameHeader h;
    if (!candidate(pos, variable, 0, &h)) return refuse("flac_index", "the first frame's header does not parse or disagrees with STREAMINFO");
    for (;;) {
        if (count >= FLAC_IN_MAX_FRAMES) return refuse("flac_index", "more than 2^24 frames");
        if (h.block > fi.frames - done) return refuse("flac_index", "the blocks hold more samples than STREAMINFO counts");
        const uint64_t next_number = variable ? (uint64_t)(done + h.block) : (uint64_t)(count + 1);
        // the next header: the first 0xFF 0xF8/0xF9 pair past this header + one byte of subframe whose header passes every check
        int64_t at = pos + h.bytes + 1, next = size;
        FlacFrameHeader hn{};
        while (at + 1 < size) {
            const void* hit = memchr(data + at, 0xFF, (size_t)(size - 1 - at));
            if (!hit) break;
            at = static_cast<const uint8_t*>(hit) - data;
            if ((data[at + 1] & 0xFE) == 0xF8 && candidate(at, variable, next_number, &hn)) {
                next = at;
                break;
            }
            ++at;
        }
        if (count < capacity) table[4 * count] = pos, table[4 * count + 1] = next - pos, table[4 * count + 2] = done, table[4 * count + 3] = h.block;
        ++count, done += h.block;
        if (next == size) break;
        pos = next, h = hn;
    }
    *n_frames = count;
    if (done != fi.frames)
        return refuse("flac_index", "the blocks sum to " + std::to_string(done) + " samples, STREAMINFO counts " + std::to_string(fi.frames));
    if (count > capacity) return refuse("flac_index", "the table holds " + std::to_string(capacity) + " rows, the stream has " + std::to_string(count) + " frames");
    return ACE355_OK;
}

int ace355_flac_in_plan(int64_t n_frames, int32_t channels, int32_t bits_per_sample, int32_t max_block, int64_t total_samples,
                        ace355_flac_in_plan_info* out) {
    ACE_CHECK(out, "flac_in_plan: null argument");
    const FlacInPlan p = plan_flac_in(FlacInRequest{n_frames, channels, bits_per_sample, max_block, total_samples});
    if (p.refusal) return refuse("flac_in_plan", p.refusal);
    out->entropy_grid = p.entropy_grid, out->restore_grid = p.restore_grid, out->finish_grid = p.finish_grid, out->desc_at = p.desc_at;
    out->frame_at = p.frame_at, out->scratch_bytes = p.scratch_bytes, out->out_bytes = p.out_bytes, out->launches = p.launches;
    out->entropy_threads = p.entropy_threads, out->entropy_lanes = p.entropy_lanes, out->restore_threads = p.restore_threads;
    out->restore_lanes = p.restore_lanes, out->finish_threads = p.finish_threads, out->finish_tiles = p.finish_tiles;
    out->status_threads = p.status_threads, out->out_format = p.out_format;
    return ACE355_OK;
}

int ace355_flac_in_decode(const ace355_flac_stream_info* info, const void* file_dev, int64_t file_bytes, const int64_t* table_dev, int64_t n_frames,
                          void* scratch_dev, int64_t scratch_bytes, void* out_dev, int64_t out_bytes, int32_t* status_dev, void* stream) {
    ACE_CHECK(info && file_dev && table_dev && scratch_dev && out_dev && status_dev, "flac_in_decode: null argument");
    const FlacInPlan p = plan_flac_in(FlacInRequest{n_frames, info->channels, info->bits_per_sample, info->max_block, info->total_samples});
    if (p.refusal) return refuse("flac_in_decode", p.refusal);
    ACE_CHECK(file_bytes > 0 && scratch_bytes >= p.scratch_bytes && out_bytes >= p.out_bytes, "flac_in_decode: the scratch or the output is smaller than the plan says");
    ACE_CHECK(((reinterpret_cast<uintptr_t>(file_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 3) == 0 && (reinterpret_cast<uintptr_t>(scratch_dev) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(table_dev) & 7) == 0,
              "flac_in_decode: the file and the output must be 4-byte aligned (the file allocated up to the next multiple of 4), the scratch 16-byte, the table 8-byte");
    FlacInArgs a{};
    a.file = static_cast<const uint8_t*>(file_dev), a.file_bytes = file_bytes, a.table = table_dev, a.frames = n_frames, a.total = info->total_samples;
    char* sc = static_cast<char*>(scratch_dev);
    a.resid = reinterpret_cast<int32_t*>(sc), a.desc = reinterpret_cast<FlacSubDesc*>(sc + p.desc_at), a.frame_words = reinterpret_cast<int32_t*>(sc + p.frame_at);
    a.out = out_dev, a.status_out = status_dev;
    a.sp = FlacStreamParams{info->channels, info->bits_per_sample, info->sample_rate, info->variable_blocks ? 1 : 0};
    a.max_block = info->max_block, a.tiles = p.finish_tiles;
    hipStream_t s = (hipStream_t)stream;
    a.lanes = p.entropy_lanes;
    hipLaunchKernelGGL(flac_entropy_kernel, dim3((unsigned)p.entropy_grid), dim3(p.entropy_threads), 0, s, a);
    ACE_LAUNCH_CHECK();
    a.lanes = p.restore_lanes;
    hipLaunchKernelGGL(flac_restore_kernel, dim3((unsigned)p.restore_grid), dim3(p.restore_threads), 0, s, a);
    ACE_LAUNCH_CHECK();
    hipLaunchKernelGGL(flac_finish_kernel, dim3((unsigned)p.finish_grid), dim3(p.finish_threads), 0, s, a);
    ACE_LAUNCH_CHECK();
    hipLaunchKernelGGL(flac_status_kernel, dim3(1), dim3(p.status_threads), 0, s, a);
    ACE_LAUNCH_CHECK();
    return ACE355_OK;
}

}  // extern "C"
