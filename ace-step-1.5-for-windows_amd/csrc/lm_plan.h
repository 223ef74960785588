// lm_plan.h - the launch decisions of the LM (lm.hip: decode attention, cache fan-out; lm_sample.hip: token selection) as data, in the
// shape of attn_plan.h / gemm_plan.h.  The decode attention: how the keys [0, len) of one sequence are cut into chunks, one workgroup per (sequence, kv head, chunk), merged afterwards in chunk order.
// plan_lm_decode is a pure function of the current length ALONE: it reads no global, no environment, makes no HIP call, and does not see
// the number of sequences - so the bits of a sequence's logits do not depend on how many others decode beside it.
#pragma once

namespace ace355 {

constexpr int LM_MAX_SEQS = 16;            // lm_batch_chunk_size 8, doubled by CFG
constexpr int LM_MAX_POSITIONS = 16384;    // the longest cache a handle may be created for (the last regime below ends here)
constexpr int LM_MAX_SPLITS = 64;          // chunks of one sequence at LM_MAX_POSITIONS
constexpr int LM_DECODE_KEY_GROUPS = 16;   // keys a workgroup of decode_attn_kernel has in flight (16 lanes x 8 dims each)

struct LmDecodePlan {
    int chunk;    // keys per workgroup, a multiple of LM_DECODE_KEY_GROUPS
    int splits;   // chunks of one sequence = ceil(len / chunk) <= LM_MAX_SPLITS; chunk c holds keys [c * chunk, min(len, (c + 1) * chunk))
};

// Three regimes: short caches are cut finely so that a two-sequence CFG pair still spreads over the chip (2 x 8 kv heads x splits
// workgroups), long ones coarsely so that the merge stays short.  A workgroup reads chunk x 512 bytes of K and V: 32 / 64 / 128 KB.
inline LmDecodePlan plan_lm_decode(int len) {
    LmDecodePlan p{};
    p.chunk = len <= 256 ? 64 : len <= 1024 ? 128 : 256;
    p.splits = len > 0 ? (len + p.chunk - 1) / p.chunk : 0;
    return p;
}

// ------------------------------------------------------------------------------------------------ cache fan-out (lm.hip)
// The cache's n_old sequences become n_new: new sequence n holds old sequence src[n].  The copy is in place, so the order matters:
// with src = [0, 0, 1, 1] destination 1 overwrites old sequence 1 while destinations 2 and 3 still read it.  plan_lm_fan_out puts the
// copies into waves, one launch each, such that no wave reads a sequence that the same or an earlier wave writes: a copy's wave is
// one more than the last wave that reads its destination.  src is non-decreasing with src[n] <= n, so every reader of old sequence n
// is a destination m > n and one walk from the last destination down settles all of them.  A destination with src[n] == n stays
// where it is and is in no wave.  Pure: no global, no environment, no HIP call.
struct LmFanOutPlan {
    int n_waves;                // launches; 0 when every sequence stays
    int wave_of[LM_MAX_SEQS];   // of destination n: its wave, or -1 for src[n] == n
};

// 0, or which rule the request breaks: 1 n_new / n_old outside 1 .. LM_MAX_SEQS, 2 a decreasing src, 3 src[n] > n (or < 0),
// 4 src[n] >= n_old.  A refused request leaves *p untouched.
inline int plan_lm_fan_out(const int* src, int n_new, int n_old, LmFanOutPlan* p) {
    if (n_new < 1 || n_new > LM_MAX_SEQS || n_old < 1 || n_old > LM_MAX_SEQS) return 1;
    for (int n = 0; n < n_new; ++n) {
        if (n > 0 && src[n] < src[n - 1]) return 2;
        if (src[n] < 0 || src[n] > n) return 3;
        if (src[n] >= n_old) return 4;
    }
    LmFanOutPlan q{};
    int after[LM_MAX_SEQS] = {};   // of old sequence n: the first wave in which it may be overwritten
    for (int n = n_new - 1; n >= 0; --n) {
        if (src[n] == n) { q.wave_of[n] = -1; continue; }
        q.wave_of[n] = after[n];
        if (after[n] + 1 > q.n_waves) q.n_waves = after[n] + 1;
        if (after[n] + 1 > after[src[n]]) after[src[n]] = after[n] + 1;
    }
    *p = q;
    return 0;
}

// ------------------------------------------------------------------------------------------------ token selection (lm_sample.hip)
// How one row of V logits is cut over workgroups: chunk c holds ids [c * chunk, min(V, (c + 1) * chunk)), per-chunk partials are combined
// in chunk order.  A pure function of V ALONE (not of the number of rows), so a row's sums have one order whatever runs beside it.  One
// regime: 8192 ids (32 KB) per workgroup - a row of the real vocabulary (217 205) is 27 workgroups, 16 rows are 432.
constexpr int LM_PICK_MAX_V = 1 << 20;
constexpr int LM_PICK_CHUNK = 8192;
constexpr int LM_PICK_MAX_CHUNKS = LM_PICK_MAX_V / LM_PICK_CHUNK;   // 128

struct LmPickPlan {
    int chunk;    // ids per workgroup
    int chunks;   // ceil(V / chunk) <= LM_PICK_MAX_CHUNKS; 0 for V outside 1 .. LM_PICK_MAX_V
};

inline LmPickPlan plan_lm_pick(int V) {
    LmPickPlan p{};
    p.chunk = LM_PICK_CHUNK;
    p.chunks = V >= 1 && V <= LM_PICK_MAX_V ? (V + p.chunk - 1) / p.chunk : 0;
    return p;
}

// ------------------------------------------------------------------------------------------------ teacher-forced scoring (lm_score.hip)
// R rows of final-norm activations against the head W [V, D]: a workgroup takes LM_SCORE_TILE_ROWS rows and one chunk of ids, walks the
// chunk in steps of LM_SCORE_STEP_IDS ids with a K loop over D in slices of LM_SCORE_K_SLICE, and leaves one partial per (row, chunk);
// the merge combines a row's partials in chunk order.  Chunk c holds ids [c * chunk, min(V, (c + 1) * chunk)).  The cut of the
// vocabulary is a function of V ALONE, and a row's arithmetic does not depend on where in a tile it sits, so a row's bits do not
// depend on R or on the rows beside it.  One regime: 1024 ids per workgroup - the real vocabulary (217 205) is 213 chunks, which fill
// the chip from one row tile on.  Row tiles are the fast grid dimension: the workgroups that share a chunk of W run side by side.
constexpr int LM_SCORE_TILE_ROWS = 64;
constexpr int LM_SCORE_STEP_IDS = 256;
constexpr int LM_SCORE_K_SLICE = 64;
constexpr int LM_SCORE_CHUNK = 1024;
constexpr int LM_SCORE_MAX_ROWS = 65536;   // ACE355_LM_MAX_TOKENS
constexpr int LM_SCORE_MAX_V = LM_PICK_MAX_V;
constexpr int LM_SCORE_MAX_D = 16384;
constexpr int LM_SCORE_PART_BYTES = 32;    // one (row, chunk) partial: max, sum, two counts, the target's logit, a flag, padding
static_assert(LM_SCORE_CHUNK % LM_SCORE_STEP_IDS == 0, "a chunk is a whole number of column steps");

struct LmScorePlan {
    int tile_rows;   // rows per workgroup
    int chunk;       // ids per workgroup
    int chunks;      // ceil(V / chunk); 0 for a request outside the limits
    int grid_x;      // row tiles = ceil(R / tile_rows)
    int grid_y;      // = chunks
};

// 0 chunks for R outside 1 .. LM_SCORE_MAX_ROWS, V outside 1 .. LM_SCORE_MAX_V, or D no multiple of LM_SCORE_K_SLICE in (0, LM_SCORE_MAX_D]
inline LmScorePlan plan_lm_score(int R, int V, int D) {
    LmScorePlan p{};
    p.tile_rows = LM_SCORE_TILE_ROWS;
    p.chunk = LM_SCORE_CHUNK;
    if (R < 1 || R > LM_SCORE_MAX_ROWS || V < 1 || V > LM_SCORE_MAX_V || D < 1 || D > LM_SCORE_MAX_D || D % LM_SCORE_K_SLICE != 0) return p;
    p.chunks = (V + p.chunk - 1) / p.chunk;
    p.grid_x = (R + p.tile_rows - 1) / p.tile_rows;
    p.grid_y = p.chunks;
    return p;
}

// the rows entry's workspace: z fp32 [R] (the counting thresholds), then the partials [R][chunks]; 0 for a request outside the limits
inline unsigned long long lm_score_align256(unsigned long long n) { return (n + 255) & ~255ull; }
inline unsigned long long lm_score_workspace_bytes(int R, int V) {
    const LmScorePlan p = plan_lm_score(R, V, LM_SCORE_K_SLICE);
    if (p.chunks == 0) return 0;
    return lm_score_align256((unsigned long long)R * 4) + lm_score_align256((unsigned long long)R * p.chunks * LM_SCORE_PART_BYTES);
}

}  // namespace ace355
