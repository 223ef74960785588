// flac_in_plan.h - the launches of the GPU FLAC decode (flac_in.hip) as data, in the shape of audio_in_plan.h: a pure function of
// (frames in the table, channels, bits per sample, STREAMINFO's max block, total samples).  It reads no global, no environment and
// makes no HIP call; ace355_flac_in_decode does exactly what it says.
//
// Four launches on one stream:
//   entropy  one LANE per frame.  A frame is serial (the second subframe starts where the first one ends), so a lane costs about
//            channels x block residuals.  Lanes of a wave follow different bitstreams: every load and store is divergent, and a wave
//            costs what its slowest lane costs however few lanes are live.  So the frames are spread over as many waves as the chip
//            has SIMDs (FLAC_IN_WAVE_SLOTS) before a second lane of any wave is used: lanes = ceil(frames / slots), 1 .. 64.
//   restore  one lane per subframe (frames x channels), spread the same way: block x order multiply-adds per lane.
//   finish   one lane per sample: `tiles` workgroups of 256 per frame, coalesced loads and stores.
//   status   one workgroup: the first frame whose status is not ok, and its code.
// Scratch: int32 residuals [channels][total] | descriptors [frames][2][FLAC_DESC_INTS] int32 | (status, assignment) [frames][2] int32.
#pragma once

#include <stdint.h>

namespace ace355 {

constexpr int FLAC_IN_WAVE_SLOTS = 1024;      // 256 CUs x 4 SIMDs: one wave each before any wave gets a second live lane
constexpr int FLAC_IN_WAVE = 64;
constexpr int FLAC_IN_FINISH_THREADS = 256;
constexpr int FLAC_IN_STATUS_THREADS = 256;
constexpr int FLAC_IN_MIN_BLOCK = 16, FLAC_IN_MAX_BLOCK = 16384;
constexpr long long FLAC_IN_MAX_FRAMES = 1ll << 24;
constexpr long long FLAC_IN_MAX_SAMPLES = 1ll << 32;   // per channel: 24 h at 48 kHz; keeps the scratch below 2^36 bytes
constexpr int FLAC_IN_DESC_INTS = 40;                  // = FLAC_DESC_INTS (flac_in.h)

struct FlacInRequest {
    long long frames;   // rows of the frame table
    int channels, bps, max_block;
    long long total;    // samples per channel
};

struct FlacInPlan {
    int launches;
    long long entropy_grid, restore_grid, finish_grid;
    int entropy_threads, entropy_lanes;   // workgroup = one wave; its first `lanes` lanes own a frame each
    int restore_threads, restore_lanes;
    int finish_threads, finish_tiles;     // finish_grid = frames x tiles; workgroup (f, t) owns samples [256 t, 256 t + 256) of frame f
    int status_threads;                   // one workgroup
    int out_format;                       // ACE355_PCM_S16 (1) at 16 bits, ACE355_PCM_S32 (3) above: left-justified, v << (32 - bps)
    long long desc_at, frame_at;          // byte offsets of the descriptors and the (status, assignment) pairs in the scratch
    long long scratch_bytes, out_bytes;   // out_bytes is a multiple of 4
    const char* refusal;
};

inline FlacInPlan plan_flac_in(const FlacInRequest& r) {
    FlacInPlan p{};
    if (r.frames < 1 || r.frames > FLAC_IN_MAX_FRAMES) return p.refusal = "frames must be 1 .. 2^24", p;
    if (r.channels < 1 || r.channels > 2) return p.refusal = "channels must be 1 or 2", p;
    if (r.bps < 16 || r.bps > 24) return p.refusal = "bits per sample must be 16 .. 24", p;
    if (r.max_block < FLAC_IN_MIN_BLOCK || r.max_block > FLAC_IN_MAX_BLOCK) return p.refusal = "the max block must be 16 .. 16384", p;
    if (r.total < 1 || r.total > FLAC_IN_MAX_SAMPLES) return p.refusal = "total samples must be 1 .. 2^32", p;
    if (r.total < r.frames || r.total > r.frames * r.max_block) return p.refusal = "frames x max block cannot hold that many samples", p;
    auto lanes = [](long long units) {
        const long long l = (units + FLAC_IN_WAVE_SLOTS - 1) / FLAC_IN_WAVE_SLOTS;
        return (int)(l < 1 ? 1 : l > FLAC_IN_WAVE ? FLAC_IN_WAVE : l);
    };
    p.launches = 4;
    p.entropy_threads = p.restore_threads = FLAC_IN_WAVE;
    p.entropy_lanes = lanes(r.frames), p.entropy_grid = (r.frames + p.entropy_lanes - 1) / p.entropy_lanes;
    const long long subframes = r.frames * r.channels;
    p.restore_lanes = lanes(subframes), p.restore_grid = (subframes + p.restore_lanes - 1) / p.restore_lanes;
    p.finish_threads = FLAC_IN_FINISH_THREADS, p.finish_tiles = (r.max_block + FLAC_IN_FINISH_THREADS - 1) / FLAC_IN_FINISH_THREADS;
    p.finish_grid = r.frames * p.finish_tiles;   // <= 2^24 x 64
    p.status_threads = FLAC_IN_STATUS_THREADS;
    p.out_format = r.bps == 16 ? 1 : 3;
    p.desc_at = (4ll * r.channels * r.total + 15) / 16 * 16;
    p.frame_at = p.desc_at + r.frames * 2 * FLAC_IN_DESC_INTS * 4;
    p.scratch_bytes = p.frame_at + r.frames * 8;
    p.out_bytes = r.bps == 16 ? (2ll * r.channels * r.total + 3) / 4 * 4 : 4ll * r.channels * r.total;
    return p;
}

}  // namespace ace355
