// audio_in_plan.h - the launch decision of the audio input stage (audio_in.hip) as data, in the shape of lm_plan.h / gemm_plan.h: how the
// 48 kHz output frames of one clip are cut into tiles, one workgroup per tile, what a tile stages in LDS, and which requests are refused.
// plan_audio_in is a pure function of the request ALONE: it reads no global, no environment, makes no HIP call.
//
// The resampler is torchaudio's windowed-sinc polyphase filter (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99): with
// g = gcd(sr, 48000), o = sr / g, n = 48000 / g, width = ceil(6 o / (min(o, n) 0.99)), output frame j = b n + p is
// sum_i k[p][i] x[b o + i - width] over the 2 width + o taps of phase p.  The host keeps, per phase, the K consecutive taps that cover
// every tap whose window argument is not clamped (the others are ~1e-33): first[p] and K floats.
#pragma once

#include <stdint.h>

namespace ace355 {

constexpr int AUDIO_IN_RATE = 48000;
constexpr int AUDIO_IN_FORMATS = 5;              // ACE355_PCM_U8 .. ACE355_PCM_F32
constexpr int AUDIO_IN_THREADS = 256;
constexpr int AUDIO_IN_MAX_TILE = 1024;          // output frames of a workgroup: 4 per thread
constexpr int AUDIO_IN_MIN_TILE = 64;
constexpr int AUDIO_IN_LDS_BYTES = 60 * 1024;    // a tile's input span (both channels, fp32) + the table when it sits in LDS
constexpr int AUDIO_IN_TABLE_LDS_BYTES = 24 * 1024;   // a compacted table up to this size is copied into LDS by every workgroup
// The cap on the table: the DENSE table n x (2 width + o) is what the host builds in fp64 before it compacts it, and what torchaudio
// would hold in fp32.  2^22 taps = 32 MB of fp64.  Every rate in use is far below (44100: 160 x 161, 11025: 640 x 161, 22255: 9600 x 4465
// is refused); a rate coprime to 48000 has 48000 phases of ~48000 taps (47999: 2.3e9, 18 GB in fp32) and stays with the host path.
constexpr long long AUDIO_IN_MAX_DENSE_TAPS = 1ll << 22;
constexpr long long AUDIO_IN_MAX_FRAMES = 1ll << 36;   // input frames (FLAC's STREAMINFO holds 36 bits); keeps n * frames inside int64
constexpr long long AUDIO_IN_MAX_GRID = 0x7fffffffll;

struct AudioInRequest {
    int format;       // ACE355_PCM_*
    int channels;     // interleaved channels of the payload, >= 1 (1 is duplicated, more than 2: channels 0 and 1)
    int o, n;         // sr / g and 48000 / g
    int K;            // taps kept per phase; 0 exactly when o == n == 1 (48 kHz: conversion, channel map and clamp only)
    int width;        // ceil(6 o / (min(o, n) 0.99)); 0 when o == n == 1
    long long frames; // L, input frames
};

struct AudioInPlan {
    long long out_frames;   // ceil(n L / o)
    long long grid;         // workgroups = ceil(out_frames / tile): tile t owns output frames [t tile, min(out_frames, (t + 1) tile))
    int tile;               // output frames per workgroup
    int threads;
    int span;               // input frames a tile stages per channel: frames [b0 o - width, + span), b0 = (t tile) / n, zero outside [0, L)
    int table_in_lds;       // the workgroup copies first[] and the taps into LDS (row stride K | 1); 0: it reads them from global memory
    int lds_bytes;          // dynamic LDS of the launch
    int passthrough;        // K == 0
    const char* refusal;    // non-null: why there is no launch (the other fields are then 0)
};

inline int audio_in_sample_bytes(int format) { return format == 0 ? 1 : format == 1 ? 2 : format == 2 ? 3 : 4; }

inline long long audio_in_gcd(long long a, long long b) {
    while (b) {
        const long long t = a % b;
        a = b, b = t;
    }
    return a;
}

inline AudioInPlan plan_audio_in(const AudioInRequest& r) {
    AudioInPlan p{};
    if (r.format < 0 || r.format >= AUDIO_IN_FORMATS) return p.refusal = "format is not one of ACE355_PCM_*", p;
    if (r.channels < 1 || r.channels > 65535) return p.refusal = "channels must be 1 .. 65535", p;
    if (r.o <= 0 || r.n <= 0) return p.refusal = "the sample rate must be positive", p;
    if (AUDIO_IN_RATE % r.n != 0 || audio_in_gcd(r.o, r.n) != 1) return p.refusal = "o / n is not a source rate over 48000 in lowest terms", p;
    if (r.frames < 1 || r.frames > AUDIO_IN_MAX_FRAMES) return p.refusal = "frames must be 1 .. 2^36", p;
    const bool pass = r.o == 1 && r.n == 1;
    const long long dense = 2ll * r.width + r.o;
    if (pass ? (r.K != 0 || r.width != 0) : (r.width < 1 || r.K < 1 || r.K > dense))
        return p.refusal = "K / width do not describe a tap table of this rate (48 kHz has none)", p;
    if (!pass && (long long)r.n * dense > AUDIO_IN_MAX_DENSE_TAPS) return p.refusal = "the tap table of this rate exceeds 2^22 dense taps", p;
    const long long out = ((long long)r.n * r.frames + r.o - 1) / r.o;
    const int kp = r.K | 1;
    const long long table_bytes = pass ? 0 : 4ll * r.n * (kp + 1);
    const bool in_lds = !pass && table_bytes <= AUDIO_IN_TABLE_LDS_BYTES;
    int tile = AUDIO_IN_MAX_TILE;
    long long span = 0, lds = 0;
    for (;; tile >>= 1) {
        // a tile's outputs sit in at most (tile + n - 2) / n + 1 blocks of n; block b reads input frames [b o - width, b o + o + width)
        span = pass ? 0 : ((long long)(tile + r.n - 2) / r.n) * r.o + dense;
        lds = 8 * span + (in_lds ? table_bytes : 0);
        if (lds <= AUDIO_IN_LDS_BYTES) break;
        if (tile == AUDIO_IN_MIN_TILE) return p.refusal = "a 64-frame tile's input span does not fit in LDS at this rate", p;
    }
    const long long grid = (out + tile - 1) / tile;
    if (grid > AUDIO_IN_MAX_GRID) return p.refusal = "the output exceeds 2^31 - 1 tiles", p;
    p.out_frames = out, p.grid = grid, p.tile = tile, p.threads = AUDIO_IN_THREADS, p.span = (int)span, p.table_in_lds = in_lds ? 1 : 0;
    p.lds_bytes = (int)lds, p.passthrough = pass ? 1 : 0;
    return p;
}

}  // namespace ace355
