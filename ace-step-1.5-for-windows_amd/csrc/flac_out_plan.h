// flac_out_plan.h - the launches of the GPU FLAC encode (flac_out.hip) as data, in the shape of flac_in_plan.h: a pure function of
// (items, frames per item, channels).  It reads no global, no environment and makes no HIP call; ace355_flac_out_encode does exactly
// what it says.
//
// Three launches on one stream:
//   frame    one workgroup of 256 per (item, block): the block's PCM in LDS, the candidates' integer sums, the partition-order search (one
//            wave per candidate), the assignment, an exclusive scan of code lengths, every lane's own codes ORed into a zeroed bit buffer
//            in LDS, CRC-16 from 256 chunk CRCs, then the frame's bytes into its slot and its byte count.
//   offsets  one workgroup per item: exclusive scan of the frame sizes; total, min, max and a status into records [n_items][4] int64.
//   gather   one workgroup per (item, block): the frame from its slot to out + item x item_stride + 42 + offset.
// Scratch: slots [units][slot_stride] bytes | sizes uint32 [units] at sizes_at | offsets int64 [units] at offsets_at.
// Output: item i's file at i x item_stride: 42 bytes the host fills (ace355_flac_streaminfo), then the frames.
#pragma once

#include <stdint.h>

#include "flac_out.h"

namespace ace355 {

constexpr int FLAC_OUT_MAX_ITEMS = 4096;
constexpr long long FLAC_OUT_MAX_FRAMES = 1ll << 36;   // STREAMINFO's sample count has 36 bits
constexpr long long FLAC_OUT_MAX_UNITS = 1ll << 21;    // (item, block) pairs: the slots stay below 2^36 bytes and a grid index holds them
constexpr int FLAC_OUT_RECORD_INTS = 4;                // int64 per item: frame bytes, min frame, max frame, status (0 = fine)

// ace355_flac_bound (audio_out.hip): the verbatim worst case.
inline long long flac_out_bound(long long frames, int channels) {
    const long long nblk = (frames + FLAC_OUT_BLOCK - 1) / FLAC_OUT_BLOCK;
    return 42 + nblk * 32 + (frames * channels * 17 + 7) / 8 + nblk * channels * 2;
}

struct FlacOutPlan {
    int launches;                                      // 3
    long long blocks, units;                           // blocks per item; n_items x blocks
    long long frame_grid, offsets_grid, gather_grid;
    int frame_threads, offsets_threads, gather_threads;
    int frame_lds_bytes, offsets_lds_bytes;
    int slot_stride;                                   // bytes of a frame's slot in the scratch
    long long item_stride;                             // bytes between two items' files in the output: the bound, up to a multiple of 16
    long long sizes_at, offsets_at;
    long long scratch_bytes, out_bytes, records_bytes;
    const char* refusal;
};

// max_units: a caller's lower ceiling on n_items x blocks (ace355_save_audio_batch_ex takes one from ACE355_FLAC_OUT_MAX_UNITS, to bound the
// scratch it allocates: 17 KB per pair); values outside 1 .. FLAC_OUT_MAX_UNITS mean FLAC_OUT_MAX_UNITS.
inline FlacOutPlan plan_flac_out(int n_items, long long frames, int channels, long long max_units = FLAC_OUT_MAX_UNITS) {
    FlacOutPlan p{};
    if (n_items < 1 || n_items > FLAC_OUT_MAX_ITEMS) return p.refusal = "n_items must be 1 .. 4096", p;
    if (channels < 1 || channels > 2) return p.refusal = "channels must be 1 or 2", p;
    if (frames < 1 || frames >= FLAC_OUT_MAX_FRAMES) return p.refusal = "frames must be 1 .. 2^36 - 1 (an empty stream is its 42 header bytes: nothing to launch)", p;
    p.blocks = (frames + FLAC_OUT_BLOCK - 1) / FLAC_OUT_BLOCK;
    p.units = p.blocks * n_items;
    if (max_units < 1 || max_units > FLAC_OUT_MAX_UNITS) max_units = FLAC_OUT_MAX_UNITS;
    if (p.units > max_units)
        return p.refusal = "n_items x blocks is above the ceiling (2^21 for the grid index and the scratch, unless the caller sets a lower one)", p;
    p.item_stride = (flac_out_bound(frames, channels) + 15) / 16 * 16;
    p.out_bytes = p.item_stride * n_items;
    p.records_bytes = 8ll * FLAC_OUT_RECORD_INTS * n_items;
    p.slot_stride = FLAC_OUT_SLOT_BYTES;
    p.launches = 3;
    p.frame_grid = p.gather_grid = p.units, p.offsets_grid = n_items;
    p.frame_threads = p.offsets_threads = p.gather_threads = FLAC_OUT_THREADS;
    p.frame_lds_bytes = (int)sizeof(FlacOutLds);
    p.offsets_lds_bytes = 4 * 4 * FLAC_OUT_WAVES;
    p.sizes_at = p.units * p.slot_stride;
    p.offsets_at = (p.sizes_at + 4 * p.units + 15) / 16 * 16;
    p.scratch_bytes = p.offsets_at + 8 * p.units;
    return p;
}

}  // namespace ace355
