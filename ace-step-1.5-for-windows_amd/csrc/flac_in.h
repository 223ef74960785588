// flac_in.h - one FLAC frame (RFC 9639), as the GPU decode of flac_in.hip and the stand-alone host program tests/flac_in_host.cpp run
// it: plain C++ without __HIPCC__, __host__ __device__ with it.  Four routines, all over a byte range [begin, begin + len) of a buffer
// that is readable up to the next multiple of 4 past its end:
//   flac_parse_frame_header   the byte-aligned header with its CRC-8
//   flac_frame_entropy        header re-parse against the table row, subframe headers, warm-up samples and residuals -> int32 scratch,
//                             one descriptor per subframe, CRC-16 over the frame
//   flac_subframe_restore     the fixed / LPC recurrence in place (int64 sums)
//   flac_finish_sample        wasted bits back, inter-channel decorrelation undone
// Memory safety on a malformed stream: every bitstream read is clamped to the frame's byte range (a dword at or past its end reads as 0
// and sets `bad` once a bit of it is consumed), every loop is bounded by the block size or by the bits left, every store goes to
// [0, block) of the frame's own scratch rows.  All sample arithmetic is unsigned, so a hostile stream wraps instead of overflowing.
#pragma once

#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define FLAC_HD __host__ __device__ inline
#else
#define FLAC_HD inline
#endif

namespace ace355 {

// per-frame status codes (ace355.h: ACE355_FLAC_*)
constexpr int FLAC_OK = 0;
constexpr int FLAC_HEADER_MISMATCH = 1;   // no sync, CRC-8, or a field that differs from its table row / STREAMINFO
constexpr int FLAC_RESERVED = 2;          // a reserved or invalid code
constexpr int FLAC_OVERRUN = 3;           // the frame wants more bits than its byte range holds
constexpr int FLAC_SAMPLE_COUNT = 4;      // the subframe does not produce `block` samples (order / partition structure)
constexpr int FLAC_CRC16 = 5;

constexpr int FLAC_KIND_CONSTANT = 0, FLAC_KIND_VERBATIM = 1, FLAC_KIND_FIXED = 2, FLAC_KIND_LPC = 3;
constexpr int FLAC_DESC_INTS = 40;

struct FlacSubDesc {   // FLAC_DESC_INTS int32
    int32_t kind, order, precision, shift, wasted, pad[3];
    int32_t coef[32];
};

struct FlacStreamParams {
    int32_t channels, bps, sample_rate, variable;   // STREAMINFO's, and the first frame's blocking-strategy bit
};

struct FlacFrameHeader {
    int32_t variable, block, sample_rate, bps, assign, channels, bytes;   // sample_rate / bps 0: "as STREAMINFO"; bytes incl. the CRC-8
    uint64_t number;                                                       // frame number (fixed blocking) or first sample (variable)
};

struct FlacCrcTables {
    uint8_t c8[256];
    uint16_t c16[256];
    constexpr FlacCrcTables() : c8(), c16() {
        for (int i = 0; i < 256; ++i) {
            uint32_t a = (uint32_t)i, b = (uint32_t)i << 8;
            for (int k = 0; k < 8; ++k) {
                a = (a & 0x80u) ? ((a << 1) ^ 0x07u) & 0xffu : (a << 1) & 0xffu;
                b = (b & 0x8000u) ? ((b << 1) ^ 0x8005u) & 0xffffu : (b << 1) & 0xffffu;
            }
            c8[i] = (uint8_t)a, c16[i] = (uint16_t)b;
        }
    }
};

// p: the first byte of the candidate; avail: bytes readable from p.  FLAC_OK and *h, or the code that rejects it.
FLAC_HD int flac_parse_frame_header(const uint8_t* p, int64_t avail, FlacFrameHeader* h) {
    constexpr FlacCrcTables T{};
    if (avail < 6) return FLAC_OVERRUN;
    if (p[0] != 0xFF || (p[1] & 0xFE) != 0xF8) return FLAC_HEADER_MISMATCH;
    h->variable = p[1] & 1;
    const int bs_code = p[2] >> 4, sr_code = p[2] & 15, assign = p[3] >> 4, ss_code = (p[3] >> 1) & 7;
    if ((p[3] & 1) || bs_code == 0 || sr_code == 15 || ss_code == 3 || assign > 10) return FLAC_RESERVED;
    int nb = 0;   // bytes of the coded number: 1 .. 7
    const uint32_t lead = p[4];
    while (nb < 8 && (lead & (0x80u >> nb))) ++nb;
    if (nb == 1 || nb == 8) return FLAC_RESERVED;   // a continuation byte, or 0xFF
    const int nbytes = nb == 0 ? 1 : nb;
    const int extra_bs = bs_code == 6 ? 1 : bs_code == 7 ? 2 : 0, extra_sr = sr_code == 12 ? 1 : (sr_code == 13 || sr_code == 14) ? 2 : 0;
    const int total = 4 + nbytes + extra_bs + extra_sr + 1;
    if (total > avail) return FLAC_OVERRUN;
    uint64_t num = nb == 0 ? lead : (lead & (0x7Fu >> nb));
    for (int i = 1; i < nbytes; ++i) {
        if ((p[4 + i] & 0xC0) != 0x80) return FLAC_RESERVED;
        num = (num << 6) | (p[4 + i] & 0x3Fu);
    }
    int at = 4 + nbytes, bs;
    if (bs_code == 1) bs = 192;
    else if (bs_code <= 5) bs = 576 << (bs_code - 2);
    else if (bs_code == 6) bs = p[at] + 1;
    else if (bs_code == 7) bs = ((p[at] << 8) | p[at + 1]) + 1;
    else bs = 256 << (bs_code - 8);
    at += extra_bs;
    int sr = 0;
    switch (sr_code) {
        case 1: sr = 88200; break;
        case 2: sr = 176400; break;
        case 3: sr = 192000; break;
        case 4: sr = 8000; break;
        case 5: sr = 16000; break;
        case 6: sr = 22050; break;
        case 7: sr = 24000; break;
        case 8: sr = 32000; break;
        case 9: sr = 44100; break;
        case 10: sr = 48000; break;
        case 11: sr = 96000; break;
        case 12: sr = p[at] * 1000; break;
        case 13: sr = (p[at] << 8) | p[at + 1]; break;
        case 14: sr = ((p[at] << 8) | p[at + 1]) * 10; break;
        default: break;
    }
    at += extra_sr;
    uint32_t c = 0;
    for (int i = 0; i < at; ++i) c = T.c8[c ^ p[i]];
    if (c != p[at]) return FLAC_HEADER_MISMATCH;
    h->block = bs, h->sample_rate = sr, h->assign = assign, h->channels = assign < 8 ? assign + 1 : 2, h->number = num, h->bytes = total;
    h->bps = ss_code == 0 ? 0 : ss_code == 1 ? 8 : ss_code == 2 ? 12 : ss_code == 4 ? 16 : ss_code == 5 ? 20 : ss_code == 6 ? 24 : 32;
    return FLAC_OK;
}

// The aligned dword d of the buffer, bytes in stream order (big endian); 0 at or past the end of the frame's range.
FLAC_HD uint32_t flac_load_be32(const uint8_t* base, int64_t d, int64_t end_byte) {
    if (d * 4 >= end_byte) return 0;
    uint32_t v;
#if defined(__HIP_DEVICE_COMPILE__)
    v = *reinterpret_cast<const uint32_t*>(base + d * 4);
#else
    memcpy(&v, base + d * 4, 4);
#endif
    return __builtin_bswap32(v);
}

// MSB-first reader over bytes [begin, end) of `base`: a 64-bit window whose top `have` bits are the next ones (the rest zero), refilled
// by one aligned dword load whenever 32 bits or fewer are left.  pos + have is always a multiple of 32.
struct FlacBits {
    const uint8_t* base;
    int64_t end_byte, end_bit, pos;
    uint64_t win;
    int have;
    bool bad;

    FLAC_HD void open(const uint8_t* b, int64_t begin, int64_t end) {
        base = b, end_byte = end, end_bit = end * 8, pos = begin * 8, bad = begin > end;
        const int skip = (int)(begin & 3) * 8;
        win = (uint64_t)flac_load_be32(base, begin >> 2, end_byte) << (32 + skip);
        have = 32 - skip;
    }
    FLAC_HD void refill() {   // have <= 32 on entry
        const uint32_t x = flac_load_be32(base, (pos + have) >> 5, end_byte);
        win |= (uint64_t)x << (32 - have);
        have += 32;
    }
    FLAC_HD uint32_t get(int n) {   // 0 <= n <= 32
        if (n == 0) return 0;
        if (have < n) refill();
        const uint32_t v = (uint32_t)(win >> (64 - n));
        win <<= n, have -= n, pos += n;
        if (pos > end_bit) bad = true;
        return v;
    }
    FLAC_HD int32_t sget(int n) {   // two's complement, n bits
        if (n == 0) return 0;
        return (int32_t)(get(n) << (32 - n)) >> (32 - n);
    }
    // zeros ahead of the next 1 bit, which is consumed too: count-leading-zeros on the window, a refill per 32 zeros at the most
    FLAC_HD uint32_t unary() {
        uint32_t q = 0;
        for (;;) {
            if (have == 0) refill();
            if (win != 0) {
                const int z = __builtin_clzll(win);   // < have: the bits below `have` are zero
                q += (uint32_t)z;
                win = (win << z) << 1, have -= z + 1, pos += z + 1;
                if (pos > end_bit) bad = true;
                return q;
            }
            q += (uint32_t)have, pos += have, have = 0;
            if (pos >= end_bit) return bad = true, q;
        }
    }
    FLAC_HD void align() {
        const int r = (int)(pos & 7);
        if (r) get(8 - r);
    }
};

// One subframe of `block` samples at `bps` bits: warm-up samples and residuals (a constant or verbatim subframe: its samples) to
// s[0 .. block), the rest to *d.  Returns a status code.
FLAC_HD int flac_subframe_entropy(FlacBits& br, int block, int bps, int32_t* s, FlacSubDesc* d) {
    if (br.get(1)) return FLAC_RESERVED;
    const int type = (int)br.get(6);
    int wasted = 0;
    if (br.get(1)) wasted = 1 + (int)br.unary();
    if (br.bad) return FLAC_OVERRUN;
    bps -= wasted;
    if (bps <= 0) return FLAC_RESERVED;
    d->wasted = wasted, d->order = 0, d->precision = 0, d->shift = 0;
    if (type == 0) {
        d->kind = FLAC_KIND_CONSTANT;
        const int32_t v = br.sget(bps);
        for (int i = 0; i < block; ++i) s[i] = v;
        return br.bad ? FLAC_OVERRUN : FLAC_OK;
    }
    if (type == 1) {
        d->kind = FLAC_KIND_VERBATIM;
        for (int i = 0; i < block && !br.bad; ++i) s[i] = br.sget(bps);
        return br.bad ? FLAC_OVERRUN : FLAC_OK;
    }
    const bool lpc = type >= 32;
    if (!lpc && !(type >= 8 && type <= 12)) return FLAC_RESERVED;
    const int order = lpc ? (type & 31) + 1 : (type & 7);
    if (order > block) return FLAC_SAMPLE_COUNT;
    d->kind = lpc ? FLAC_KIND_LPC : FLAC_KIND_FIXED, d->order = order;
    for (int i = 0; i < order; ++i) s[i] = br.sget(bps);
    if (lpc) {
        const int prec = (int)br.get(4) + 1, shift = br.sget(5);
        if (prec == 16 || shift < 0) return FLAC_RESERVED;
        d->precision = prec, d->shift = shift;
        for (int i = 0; i < order; ++i) d->coef[i] = br.sget(prec);
    }
    const int method = (int)br.get(2);
    if (br.bad) return FLAC_OVERRUN;
    if (method > 1) return FLAC_RESERVED;
    const int kbits = method == 0 ? 4 : 5, esc = method == 0 ? 15 : 31;
    const int po = (int)br.get(4), len = block >> po;
    if (po > 0 && ((len << po) != block || len < order)) return FLAC_SAMPLE_COUNT;
    int i = order;
    for (int p = 0; p < (1 << po); ++p) {
        const int k = (int)br.get(kbits), end = (p + 1) * len;
        if (k == esc) {
            const int raw = (int)br.get(5);
            for (; i < end && !br.bad; ++i) s[i] = br.sget(raw);
        } else {
            for (; i < end && !br.bad; ++i) {
                const uint32_t q = br.unary();
                const uint32_t u = (q << k) | br.get(k);
                s[i] = (int32_t)((u >> 1) ^ (0u - (u & 1u)));
            }
        }
        if (br.bad) return FLAC_OVERRUN;
    }
    return FLAC_OK;
}

FLAC_HD uint32_t flac_crc16(const uint8_t* base, int64_t begin, int64_t end) {
    constexpr FlacCrcTables T{};
    uint32_t c = 0;
    int64_t i = begin;
    for (; i < end && (i & 3); ++i) c = ((c << 8) & 0xffffu) ^ T.c16[(c >> 8) ^ base[i]];
    for (; i + 4 <= end; i += 4) {
        const uint32_t w = flac_load_be32(base, i >> 2, end);
        c = ((c << 8) & 0xffffu) ^ T.c16[(c >> 8) ^ (w >> 24)];
        c = ((c << 8) & 0xffffu) ^ T.c16[(c >> 8) ^ ((w >> 16) & 0xffu)];
        c = ((c << 8) & 0xffffu) ^ T.c16[(c >> 8) ^ ((w >> 8) & 0xffu)];
        c = ((c << 8) & 0xffffu) ^ T.c16[(c >> 8) ^ (w & 0xffu)];
    }
    for (; i < end; ++i) c = ((c << 8) & 0xffffu) ^ T.c16[(c >> 8) ^ base[i]];
    return c;
}

// The entropy pass of one frame: bytes [begin, begin + len) of `base`, expected to hold the frame the table row describes (`block`
// samples; coded number `number`: the frame's index, or its first sample in a variable-blocksize stream).  c0 / c1: the frame's
// scratch rows (c1 unused in mono), d[0 .. channels): its descriptors, *assign: its channel assignment.
FLAC_HD int flac_frame_entropy(const uint8_t* base, int64_t begin, int64_t len, uint64_t number, int block, const FlacStreamParams& sp,
                               int32_t* c0, int32_t* c1, FlacSubDesc* d, int32_t* assign) {
    FlacFrameHeader h;
    if (len < 2) return FLAC_OVERRUN;
    const int64_t end = begin + len - 2;   // the CRC-16 is not subframe data
    const int hs = flac_parse_frame_header(base + begin, end - begin, &h);
    if (hs != FLAC_OK) return hs;
    if (h.variable != sp.variable || h.block != block || h.number != number || h.channels != sp.channels ||
        (h.sample_rate != 0 && h.sample_rate != sp.sample_rate) || (h.bps != 0 && h.bps != sp.bps))
        return FLAC_HEADER_MISMATCH;
    *assign = h.assign;
    FlacBits br;
    br.open(base, begin + h.bytes, end);
    for (int c = 0; c < h.channels; ++c) {
        const bool side = (h.assign == 8 && c == 1) || (h.assign == 9 && c == 0) || (h.assign == 10 && c == 1);
        const int st = flac_subframe_entropy(br, block, sp.bps + (side ? 1 : 0), c == 0 ? c0 : c1, d + c);
        if (st != FLAC_OK) return st;
    }
    br.align();
    if (br.bad) return FLAC_OVERRUN;
    const int64_t stop = br.pos >> 3;   // <= end
    const uint32_t want = ((uint32_t)base[stop] << 8) | base[stop + 1];
    if (flac_crc16(base, begin, stop) != want) return FLAC_CRC16;
    return stop == end ? FLAC_OK : FLAC_HEADER_MISMATCH;   // a whole frame, but not the range of its row
}

// The restore pass of one subframe, in place.  LPC sums in int64: 32 terms of a 15-bit coefficient times a 25-bit sample exceed int32.
FLAC_HD void flac_subframe_restore(int32_t* s, int block, const FlacSubDesc* d) {
    const int order = d->order;
    if (order < 0 || order > 32 || order > block) return;
    if (d->kind == FLAC_KIND_LPC) {
        const int shift = d->shift & 31;
        for (int j = order; j < block; ++j) {
            int64_t acc = 0;
            for (int c = 0; c < order; ++c) acc += (int64_t)d->coef[c] * s[j - 1 - c];
            s[j] = (int32_t)((uint32_t)s[j] + (uint32_t)(acc >> shift));
        }
    } else if (d->kind == FLAC_KIND_FIXED) {
        uint32_t a = order > 0 ? (uint32_t)s[order - 1] : 0, b = order > 1 ? (uint32_t)s[order - 2] : 0;
        uint32_t c = order > 2 ? (uint32_t)s[order - 3] : 0, e = order > 3 ? (uint32_t)s[order - 4] : 0;
        for (int j = order; j < block; ++j) {
            uint32_t v = (uint32_t)s[j];
            switch (order) {
                case 1: v += a; break;
                case 2: v += 2u * a - b; break;
                case 3: v += 3u * a - 3u * b + c; break;
                case 4: v += 4u * a - 6u * b + 4u * c - e; break;
                default: break;
            }
            s[j] = (int32_t)v;
            e = c, c = b, b = a, a = v;
        }
    }
}

// The finish pass of one sample: restored subframe values a0 / a1 -> the two channels (r unused in mono).
FLAC_HD void flac_finish_sample(int32_t a0, int32_t a1, int wasted0, int wasted1, int assign, int32_t* l, int32_t* r) {
    const uint32_t v0 = (uint32_t)a0 << (wasted0 & 31), v1 = (uint32_t)a1 << (wasted1 & 31);
    if (assign == 8) *l = (int32_t)v0, *r = (int32_t)(v0 - v1);
    else if (assign == 9) *l = (int32_t)(v0 + v1), *r = (int32_t)v1;
    else if (assign == 10) {
        const uint32_t m = (v0 << 1) | (v1 & 1u);
        *l = (int32_t)(m + v1) >> 1, *r = (int32_t)(m - v1) >> 1;
    } else *l = (int32_t)v0, *r = (int32_t)v1;
}

}  // namespace ace355

