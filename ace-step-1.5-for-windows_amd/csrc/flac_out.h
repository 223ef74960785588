// flac_out.h - one FLAC frame (RFC 9639) written the way the host encoder of audio_out.hip writes it, byte for byte, as the GPU encode of
// flac_out.hip and the stand-alone host program tests/flac_out_host.cpp run it: plain C++ without __HIPCC__, __host__ __device__ with it.
// A frame is cut over FLAC_OUT_THREADS lanes; lane t owns samples [16 t, 16 t + 16) of the block.  Every routine takes the lane's samples
// (with the four before them) and is exact integer arithmetic, so the sums do not depend on the order the lanes arrive in:
//   flac_out_lane_signal / _stats       the candidate signal (L, R, M, S), its five sum |d| over i >= 4 and "differs from sample 0"
//   flac_out_pick_order / _max_porder   lowest order wins a tie; the `while` rule of the host's plan_subframe
//   flac_out_lane_partition_sums        folded residuals into the finest partitions
//   flac_out_partition_search           from the finest order down, strict <, best_rice over k = 0 .. 14 with strict <
//   flac_out_finish_plan                constant / verbatim / fixed by fixed_bits < verbatim_bits
//   flac_out_pick_assignment            L/R, L/S, S/R, M/S in that order with strict <, on the estimated sizes
//   flac_out_frame_header               sync, block-size codes 12 / 6 / 7, sample-rate forms, coded frame number, CRC-8
//   flac_out_lane_subframe              code lengths (Write = false) and code bits (Write = true) of the lane's samples
//   flac_out_crc16_words / _shift       CRC-16 (0x8005, init 0) of a chunk, and that CRC moved past n more bytes: crc(A | B) =
//                                       shift(crc(A), |B|) ^ crc(B), so a frame's CRC is the xor of its chunks' shifted CRCs
// The bit buffer is an array of 32-bit words, bit 31 of word 0 first; a put ORs into at most two words, so only the 1 that ends a unary
// run and the k remainder bits are written into a zeroed buffer.
#pragma once

#include <stdint.h>

#include "flac_in.h"   // FLAC_HD, FlacCrcTables

#ifdef __HIPCC__
#define FLAC_OUT_UNROLL _Pragma("unroll")
#else
#define FLAC_OUT_UNROLL
#endif

namespace ace355 {

constexpr int FLAC_OUT_BLOCK = 4096;
constexpr int FLAC_OUT_THREADS = 256;
constexpr int FLAC_OUT_PER_LANE = FLAC_OUT_BLOCK / FLAC_OUT_THREADS;       // 16
constexpr int FLAC_OUT_SLOT_BYTES = FLAC_OUT_BLOCK * 2 * 17 / 8 + 64;      // the host's FrameScratch: 17472, a multiple of 16
constexpr int FLAC_OUT_SLOT_WORDS = FLAC_OUT_SLOT_BYTES / 4;
constexpr int FLAC_OUT_PCM_WORDS = FLAC_OUT_BLOCK + FLAC_OUT_BLOCK / 16;   // one pad word per 16: lanes 16 words apart hit different banks
constexpr int FLAC_OUT_MAX_PARTS = 256;
constexpr int FLAC_OUT_WAVES = FLAC_OUT_THREADS / 64;

struct FlacOutSub {
    int32_t type, order, porder, maxp;   // type 0 constant, 1 verbatim, 2 fixed
    uint64_t bits;                       // estimated size
    uint8_t k[FLAC_OUT_MAX_PARTS];
};

// What one frame's workgroup keeps in LDS (the plan reports its size).
struct FlacOutLds {
    uint32_t pcm[FLAC_OUT_PCM_WORDS];    // stereo: l | r << 16; mono: the sample; word of sample i at flac_out_pcm_at(i)
    uint32_t bits[FLAC_OUT_SLOT_WORDS];
    unsigned long long sums[4][2][FLAC_OUT_MAX_PARTS];
    FlacOutSub sub[4];
    uint8_t ks[4][FLAC_OUT_MAX_PARTS];
    unsigned long long tot[4][5];
    uint32_t differs[4];
    uint32_t scan[2][FLAC_OUT_WAVES];
    uint32_t crc[FLAC_OUT_WAVES];
    uint32_t hdr_bytes, pad;
};

FLAC_HD int flac_out_pcm_at(int i) { return i + (i >> 4); }
FLAC_HD uint32_t flac_out_fold(int32_t r) { return ((uint32_t)r << 1) ^ (uint32_t)(r >> 31); }

FLAC_HD int32_t flac_out_candidate(uint32_t word, int channels, int c) {
    const int32_t l = (int16_t)(word & 0xffffu), r = (int16_t)(word >> 16);
    if (channels == 1) return l;
    return c == 0 ? l : c == 1 ? r : c == 2 ? (l + r) >> 1 : l - r;
}

// s[j] = candidate c at sample i0 - 4 + j, 0 outside the block.
FLAC_HD void flac_out_lane_signal(const uint32_t* pcm, int channels, int c, int i0, int n, int32_t s[FLAC_OUT_PER_LANE + 4]) {
FLAC_OUT_UNROLL
    for (int j = 0; j < FLAC_OUT_PER_LANE + 4; ++j) {
        const int i = i0 - 4 + j;
        s[j] = (i >= 0 && i < n) ? flac_out_candidate(pcm[flac_out_pcm_at(i)], channels, c) : 0;
    }
}

FLAC_HD int32_t flac_out_residual(const int32_t* p, int order) {
    switch (order) {
        case 0: return p[0];
        case 1: return p[0] - p[-1];
        case 2: return p[0] - 2 * p[-1] + p[-2];
        case 3: return p[0] - 3 * p[-1] + 3 * p[-2] - p[-3];
        default: return p[0] - 4 * p[-1] + 6 * p[-2] - 4 * p[-3] + p[-4];
    }
}

// The lane's share of the five sum |d| (i >= 4 only) and of "samples that differ from the block's first".  Per lane they fit 32 bits
// (|d4| <= 2^20 on a 17-bit signal, 16 samples), and so does a wave's sum.
FLAC_HD void flac_out_lane_stats(const int32_t s[FLAC_OUT_PER_LANE + 4], int i0, int n, int32_t first, uint32_t tot[5], uint32_t* differs) {
    for (int o = 0; o < 5; ++o) tot[o] = 0;
    *differs = 0;
FLAC_OUT_UNROLL
    for (int j = 0; j < FLAC_OUT_PER_LANE; ++j) {
        const int i = i0 + j;
        if (i >= n) break;
        const int32_t* p = s + 4 + j;
        *differs += p[0] != first;
        if (i < 4) continue;
FLAC_OUT_UNROLL
        for (int o = 0; o < 5; ++o) {
            const int32_t d = flac_out_residual(p, o);
            tot[o] += (uint32_t)(d < 0 ? -d : d);
        }
    }
}

FLAC_HD int flac_out_pick_order(const uint64_t tot[5]) {
    int order = 0;
    for (int o = 1; o <= 4; ++o)
        if (tot[o] < tot[order]) order = o;
    return order;
}

FLAC_HD int flac_out_max_porder(int n, int order) {
    int maxp = 0;
    while (maxp < 8 && ((n >> (maxp + 1)) << (maxp + 1)) == n && (n >> (maxp + 1)) > order) ++maxp;
    return maxp;
}

FLAC_HD uint64_t flac_out_best_rice(uint64_t n, uint64_t sum, int* k_out) {
    uint64_t best = ~0ull;
    int bk = 0;
    for (int k = 0; k <= 14; ++k) {
        const uint64_t b = n * (uint64_t)(k + 1) + (sum >> k);
        if (b < best) best = b, bk = k;
    }
    *k_out = bk;
    return best + 4;
}

// add(partition, sum of the folded residuals of the lane's samples in it); plen = n >> maxp.
template <class Add>
FLAC_HD void flac_out_lane_partition_sums(const int32_t s[FLAC_OUT_PER_LANE + 4], int i0, int n, int order, int plen, Add&& add) {
    if (i0 >= n) return;
    int part = i0 / plen, next = (part + 1) * plen, cur = -1;
    uint64_t acc = 0;
FLAC_OUT_UNROLL
    for (int j = 0; j < FLAC_OUT_PER_LANE; ++j) {
        const int i = i0 + j;
        if (i >= n) break;
        if (i == next) ++part, next += plen;
        if (i < order) continue;
        if (part != cur) {
            if (cur >= 0) add(cur, acc);
            cur = part, acc = 0;
        }
        acc += flac_out_fold(flac_out_residual(s + 4 + j, order));
    }
    if (cur >= 0) add(cur, acc);
}

// `lanes` lanes share the search of one candidate: lane `lane` owns partitions lane, lane + lanes, ...  cx.sum(v) returns the sum of v over
// the lanes to every lane, cx.sync() makes the lanes' stores visible to each other.  sa holds the 1 << maxp finest sums; sa and sb are used
// up.  Returns the best estimate; *porder and k[0 .. 1 << *porder) are the choice (each lane writes the k of its own partitions).
template <class Ctx>
FLAC_HD uint64_t flac_out_partition_search(unsigned long long* sa, unsigned long long* sb, uint8_t* ks, uint8_t* k, int n, int order, int maxp,
                                           int lane, int lanes, Ctx&& cx, int* porder) {
    uint64_t best = ~0ull;
    int bpo = 0;
    unsigned long long *cur = sa, *nxt = sb;
    for (int po = maxp; po >= 0; --po) {
        const int cnt = 1 << po, len = n >> po;
        uint64_t bits = 0;
        for (int p = lane; p < cnt; p += lanes) {
            int kk;
            bits += flac_out_best_rice((uint64_t)(len - (p == 0 ? order : 0)), cur[p], &kk);
            ks[p] = (uint8_t)kk;
        }
        bits = cx.sum(bits);
        if (bits < best) {
            best = bits, bpo = po;
            for (int p = lane; p < cnt; p += lanes) k[p] = ks[p];
        }
        for (int p = lane; p < cnt / 2; p += lanes) nxt[p] = cur[2 * p] + cur[2 * p + 1];
        cx.sync();
        unsigned long long* t = cur;
        cur = nxt, nxt = t;
    }
    *porder = bpo;
    return best;
}

FLAC_HD void flac_out_finish_plan(FlacOutSub* pl, int n, int bps, bool constant, int order, int maxp, int porder, uint64_t best) {
    pl->order = 0, pl->porder = 0, pl->maxp = maxp;
    if (constant) {
        pl->type = 0, pl->bits = 8 + (uint64_t)bps;
        return;
    }
    const uint64_t verbatim_bits = 8 + (uint64_t)n * bps;
    pl->type = 1, pl->bits = verbatim_bits;
    if (n <= 4) return;
    const uint64_t fixed_bits = 8 + (uint64_t)order * bps + 6 + best;
    if (fixed_bits < verbatim_bits) pl->type = 2, pl->order = order, pl->porder = porder, pl->bits = fixed_bits;
}

// bits of L, R, M, S -> the assignment code and the two candidates it codes.
FLAC_HD int flac_out_pick_assignment(const uint64_t b[4], int* c0, int* c1) {
    int assign = 1;
    uint64_t best = b[0] + b[1];
    *c0 = 0, *c1 = 1;
    if (b[0] + b[3] < best) best = b[0] + b[3], assign = 8, *c0 = 0, *c1 = 3;
    if (b[3] + b[1] < best) best = b[3] + b[1], assign = 9, *c0 = 3, *c1 = 1;
    if (b[2] + b[3] < best) best = b[2] + b[3], assign = 10, *c0 = 2, *c1 = 3;
    return assign;
}

FLAC_HD int flac_out_sample_rate_code(int sr, int* extra_bytes, uint32_t* extra) {
    const int rates[11] = {88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
    *extra_bytes = 0, *extra = 0;
    for (int i = 0; i < 11; ++i)
        if (rates[i] == sr) return i + 1;
    if (sr % 1000 == 0 && sr / 1000 < 256) return *extra_bytes = 1, *extra = (uint32_t)(sr / 1000), 12;
    if (sr < 65536) return *extra_bytes = 2, *extra = (uint32_t)sr, 13;
    if (sr % 10 == 0 && sr / 10 < 65536) return *extra_bytes = 2, *extra = (uint32_t)(sr / 10), 14;
    return 0;   // "see STREAMINFO"
}

// put(i, byte) for every header byte in order, the CRC-8 last; returns the byte count (6 .. 16).  assign: 0 for mono.
template <class PutByte>
FLAC_HD int flac_out_frame_header(int n, int assign, int sample_rate, uint64_t frame_no, PutByte&& put) {
    constexpr FlacCrcTables T{};
    int at = 0;
    uint8_t crc = 0;
    auto emit = [&](uint32_t v) {
        crc = T.c8[crc ^ (uint8_t)v];
        put(at++, (uint8_t)v);
    };
    int sr_bytes;
    uint32_t sr_extra;
    const int sr_code = flac_out_sample_rate_code(sample_rate, &sr_bytes, &sr_extra);
    const int bs_code = n == FLAC_OUT_BLOCK ? 12 : (n <= 256 ? 6 : 7);
    emit(0xFF), emit(0xF8);
    emit((uint32_t)((bs_code << 4) | sr_code));
    emit((uint32_t)((assign << 4) | (4 << 1)));
    if (frame_no < 0x80) {
        emit((uint32_t)frame_no);
    } else {
        int nb = 2;
        while (nb < 7 && (frame_no >> (5 * nb + 1)) != 0) ++nb;
        emit(((0xFF00u >> nb) & 0xFF) | (uint32_t)(frame_no >> (6 * (nb - 1))));
        for (int i = nb - 2; i >= 0; --i) emit(0x80u | (uint32_t)((frame_no >> (6 * i)) & 0x3F));
    }
    if (bs_code == 6) emit((uint32_t)(n - 1));
    if (bs_code == 7) emit((uint32_t)(n - 1) >> 8), emit((uint32_t)(n - 1) & 0xFF);
    if (sr_bytes == 2) emit(sr_extra >> 8);
    if (sr_bytes) emit(sr_extra & 0xFF);
    const uint8_t c = crc;
    put(at++, c);
    return at;
}

// v's low nbits (1 .. 32) at bit `pos` of a zeroed word array, MSB first; puts past `words` are dropped.  On the device the words are in
// LDS and lanes share them: an integer OR commutes, so the bytes do not depend on the order.
FLAC_HD void flac_out_put(uint32_t* buf, int words, uint32_t pos, uint32_t v, int nbits) {
    const int w = (int)(pos >> 5), room = 32 - (int)(pos & 31);
    if (nbits < 32) v &= (1u << nbits) - 1u;
    uint32_t a, b = 0;
    if (nbits <= room) {
        a = v << (room - nbits);
    } else {
        const int r = nbits - room;
        a = v >> r, b = v << (32 - r);
    }
#if defined(__HIP_DEVICE_COMPILE__)
    if (w < words && a) atomicOr(buf + w, a);
    if (w + 1 < words && b) atomicOr(buf + w + 1, b);
#else
    if (w < words) buf[w] |= a;
    if (w + 1 < words) buf[w + 1] |= b;
#endif
}

// The lane's samples of one subframe, starting at bit `pos`: returns the bits they take; Write = true also puts them.  Sample 0 carries
// the subframe header, sample `order` the coding method and partition order, a partition's first residual its Rice parameter.
template <bool Write>
FLAC_HD uint32_t flac_out_lane_subframe(const int32_t s[FLAC_OUT_PER_LANE + 4], int i0, int n, int bps, const FlacOutSub* pl, uint32_t pos,
                                        uint32_t* buf, int words) {
    if (i0 >= n) return 0;
    uint32_t at = pos;
    auto emit = [&](uint32_t v, int nb) {
        if (Write) flac_out_put(buf, words, at, v, nb);
        at += (uint32_t)nb;
    };
    const int type = pl->type, order = pl->order, plen = n >> pl->porder;
    int part = i0 / plen, next = (part + 1) * plen;
FLAC_OUT_UNROLL
    for (int j = 0; j < FLAC_OUT_PER_LANE; ++j) {
        const int i = i0 + j;
        if (i >= n) break;
        const int32_t* p = s + 4 + j;
        if (i == next) ++part, next += plen;
        if (i == 0) emit(type == 0 ? 0x00u : type == 1 ? 0x02u : (uint32_t)((0x08 | order) << 1), 8);
        if (type == 0) {
            if (i == 0) emit((uint32_t)p[0], bps);
        } else if (type == 1 || i < order) {
            emit((uint32_t)p[0], bps);
        } else {
            if (i == order) emit((uint32_t)pl->porder, 6);   // 2 bits: Rice coding with 4-bit parameters; 4 bits: the partition order
            const int k = pl->k[part];
            if (i == order || i == part * plen) emit((uint32_t)k, 4);
            const uint32_t u = flac_out_fold(flac_out_residual(p, order));
            at += u >> k;                                     // the unary run's zeros are the buffer's
            emit((1u << k) | (u & ((1u << k) - 1u)), k + 1);
        }
    }
    return at - pos;
}

// CRC-16 of bytes [begin, end) of the word array (byte 0 = bits 31 .. 24 of word 0); begin is a multiple of 4.
FLAC_HD uint32_t flac_out_crc16_words(const uint32_t* buf, int begin, int end) {
    constexpr FlacCrcTables T{};
    uint32_t c = 0;
    for (int b = begin; b < end; b += 4) {
        const uint32_t w = buf[b >> 2];
        const int m = end - b < 4 ? end - b : 4;
        for (int i = 0; i < m; ++i) c = ((c << 8) & 0xffffu) ^ T.c16[(c >> 8) ^ ((w >> (24 - 8 * i)) & 0xffu)];
    }
    return c;
}

FLAC_HD uint32_t flac_out_gf_mul(uint32_t a, uint32_t b) {   // polynomials over GF(2) mod x^16 + x^15 + x^2 + 1
    uint32_t r = 0;
    for (int i = 15; i >= 0; --i) {
        r <<= 1;
        if (r & 0x10000u) r ^= 0x18005u;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

// The CRC of a message followed by nbytes more, given the message's CRC and zeros for the rest: crc * x^(8 nbytes).
FLAC_HD uint32_t flac_out_crc16_shift(uint32_t crc, uint32_t nbytes) {
    uint32_t f = 1, base = 0x100u;   // x^8
    for (; nbytes; nbytes >>= 1) {
        if (nbytes & 1u) f = flac_out_gf_mul(f, base);
        base = flac_out_gf_mul(base, base);
    }
    return flac_out_gf_mul(crc, f);
}

// The 42 bytes ahead of the first frame: "fLaC" and a last-block STREAMINFO.  md5 may be null: 16 zero bytes, "not computed".
inline void flac_out_streaminfo(uint8_t out[42], int64_t frames, int channels, int sample_rate, uint32_t min_frame, uint32_t max_frame,
                                const uint8_t* md5) {
    const uint8_t head[12] = {'f', 'L', 'a', 'C', 0x80, 0, 0, 34, (uint8_t)(FLAC_OUT_BLOCK >> 8), (uint8_t)FLAC_OUT_BLOCK, (uint8_t)(FLAC_OUT_BLOCK >> 8),
                              (uint8_t)FLAC_OUT_BLOCK};
    for (int i = 0; i < 12; ++i) out[i] = head[i];
    out[12] = (uint8_t)(min_frame >> 16), out[13] = (uint8_t)(min_frame >> 8), out[14] = (uint8_t)min_frame;
    out[15] = (uint8_t)(max_frame >> 16), out[16] = (uint8_t)(max_frame >> 8), out[17] = (uint8_t)max_frame;
    const uint64_t v = ((uint64_t)((uint32_t)sample_rate & 0xFFFFFu) << 44) | ((uint64_t)(channels - 1) << 41) | (15ull << 36) |
                       ((uint64_t)frames & 0xFFFFFFFFFull);
    for (int i = 0; i < 8; ++i) out[18 + i] = (uint8_t)(v >> (56 - 8 * i));
    for (int i = 0; i < 16; ++i) out[26 + i] = md5 ? md5[i] : 0;
}

}  // namespace ace355
