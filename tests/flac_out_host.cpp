// flac_out_host.cpp - the per-frame routines of csrc/flac_out.h, called in the order and with the arguments the frame kernel of
// csrc/flac_out.hip uses, with the 256 lanes of a workgroup run one after the other on the CPU by a stand-alone program
// (tests/test_flac_out_cpu.py builds it with -fsanitize=address,undefined and runs it directly).
//   flac_out_host FILE...   every case's stream equals the expected one byte for byte; per case one line
//                           "<file>: equal frames=F assign=.. types=.. orders=.. porders=.. kmax=K run=R numbytes=N"
//                           with the sets of choices its frames made, the longest unary run in bits and the longest coded frame number
// A case file (little endian): int64 channels, sample_rate, frames, expected_bytes; int16 pcm[frames][channels]; the expected stream (the
// host encoder's).  STREAMINFO's MD5 is not a routine of flac_out.h: the 16 bytes are taken from the expected stream.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "../ace-step-1.5-for-windows_amd/csrc/flac_out.h"
#include "../ace-step-1.5-for-windows_amd/csrc/flac_out_plan.h"

using namespace ace355;

struct Choices {
    std::set<int> assign, types, orders, porders;
    int kmax = 0, numbytes = 0;
    uint32_t run = 0;
};

struct OneLane {   // the search's context when one lane owns every partition
    uint64_t sum(uint64_t v) const { return v; }
    void sync() const {}
};

// One frame as flac_out_frame_kernel makes it.  pcm: the block's first sample.  Returns the frame's bytes.
static std::vector<uint8_t> encode_frame(const int16_t* pcm, int n, int channels, int sample_rate, uint64_t frame_no, Choices* ch) {
    const int T = FLAC_OUT_THREADS, ncand = channels == 2 ? 4 : 1;
    std::vector<uint32_t> words((size_t)flac_out_pcm_at(n - 1) + 1, 0), bits((size_t)FLAC_OUT_SLOT_WORDS, 0);   // exact sizes: the sanitizer sees an overrun
    for (int i = 0; i < n; ++i)
        words[(size_t)flac_out_pcm_at(i)] = channels == 2 ? ((uint32_t)(uint16_t)pcm[2 * i] | ((uint32_t)(uint16_t)pcm[2 * i + 1] << 16)) : (uint32_t)(uint16_t)pcm[i];
    std::vector<unsigned long long> sa((size_t)FLAC_OUT_MAX_PARTS), sb((size_t)FLAC_OUT_MAX_PARTS);
    std::vector<uint8_t> ks((size_t)FLAC_OUT_MAX_PARTS);
    FlacOutSub sub[4];
    int32_t s[FLAC_OUT_PER_LANE + 4];
    for (int c = 0; c < ncand; ++c) {
        uint64_t tot[5] = {0, 0, 0, 0, 0}, differs = 0;
        for (int t = 0; t < T; ++t) {
            uint32_t lt[5], ld;
            flac_out_lane_signal(words.data(), channels, c, FLAC_OUT_PER_LANE * t, n, s);
            flac_out_lane_stats(s, FLAC_OUT_PER_LANE * t, n, flac_out_candidate(words[0], channels, c), lt, &ld);
            for (int o = 0; o < 5; ++o) tot[o] += lt[o];
            differs += ld;
        }
        const bool constant = differs == 0;
        int order = 0, maxp = 0, porder = 0;
        uint64_t best = 0;
        memset(&sub[c], 0, sizeof(sub[c]));
        if (!constant && n > 4) {
            order = flac_out_pick_order(tot), maxp = flac_out_max_porder(n, order);
            std::fill(sa.begin(), sa.end(), 0ull);
            for (int t = 0; t < T; ++t) {
                flac_out_lane_signal(words.data(), channels, c, FLAC_OUT_PER_LANE * t, n, s);
                flac_out_lane_partition_sums(s, FLAC_OUT_PER_LANE * t, n, order, n >> maxp, [&](int p, uint64_t v) { sa.at((size_t)p) += v; });
            }
            best = flac_out_partition_search(sa.data(), sb.data(), ks.data(), sub[c].k, n, order, maxp, 0, 1, OneLane{}, &porder);
        }
        flac_out_finish_plan(&sub[c], n, c == 3 ? 17 : 16, constant, order, maxp, porder, best);
    }
    int assign = 0, cand[2] = {0, 0};
    if (channels == 2) {
        const uint64_t b[4] = {sub[0].bits, sub[1].bits, sub[2].bits, sub[3].bits};
        assign = flac_out_pick_assignment(b, &cand[0], &cand[1]);
    }
    const int hdr_bytes = flac_out_frame_header(n, assign, sample_rate, frame_no, [&](int i, uint8_t v) { flac_out_put(bits.data(), FLAC_OUT_SLOT_WORDS, 8u * (uint32_t)i, v, 8); });
    uint32_t at = 8u * (uint32_t)hdr_bytes;
    for (int j = 0; j < channels; ++j) {
        const FlacOutSub* pl = &sub[cand[j]];
        const int bps = cand[j] == 3 ? 17 : 16;
        std::vector<uint32_t> len((size_t)T);
        for (int t = 0; t < T; ++t) {
            flac_out_lane_signal(words.data(), channels, cand[j], FLAC_OUT_PER_LANE * t, n, s);
            len[(size_t)t] = flac_out_lane_subframe<false>(s, FLAC_OUT_PER_LANE * t, n, bps, pl, 0, nullptr, 0);
        }
        for (int t = T - 1; t >= 0; --t) {   // (any lane order: the puts commute)
            uint32_t before = 0;
            for (int u = 0; u < t; ++u) before += len[(size_t)u];
            flac_out_lane_signal(words.data(), channels, cand[j], FLAC_OUT_PER_LANE * t, n, s);
            const uint32_t wrote = flac_out_lane_subframe<true>(s, FLAC_OUT_PER_LANE * t, n, bps, pl, at + before, bits.data(), FLAC_OUT_SLOT_WORDS);
            if (wrote != len[(size_t)t]) fprintf(stderr, "lane %d: wrote %u bits, counted %u\n", t, wrote, len[(size_t)t]);
        }
        for (int t = 0; t < T; ++t) at += len[(size_t)t];
        ch->types.insert(pl->type);
        if (pl->type == 2) {
            ch->orders.insert(pl->order), ch->porders.insert(pl->porder);
            for (int p = 0; p < (1 << pl->porder); ++p) ch->kmax = pl->k[p] > ch->kmax ? pl->k[p] : ch->kmax;
            const int plen = n >> pl->porder;
            std::vector<int32_t> sig((size_t)n + 4, 0);
            for (int i = 0; i < n; ++i) sig[(size_t)i + 4] = flac_out_candidate(words[(size_t)flac_out_pcm_at(i)], channels, cand[j]);
            for (int i = pl->order; i < n; ++i) {
                const uint32_t q = flac_out_fold(flac_out_residual(sig.data() + 4 + i, pl->order)) >> pl->k[i / plen];
                ch->run = q + 1 > ch->run ? q + 1 : ch->run;
            }
        }
    }
    ch->assign.insert(assign);
    int nb = 1;
    if (frame_no >= 0x80)
        for (nb = 2; nb < 7 && (frame_no >> (5 * nb + 1)) != 0;) ++nb;
    ch->numbytes = nb > ch->numbytes ? nb : ch->numbytes;
    const int body = (int)((at + 7) >> 3);
    const int chunk = 4 * ((((body + 3) >> 2) + T - 1) / T);
    uint32_t crc = 0;
    for (int t = 0; t < T; ++t) {
        const int b0 = t * chunk, b1 = b0 + chunk < body ? b0 + chunk : body;
        if (b0 < b1) crc ^= flac_out_crc16_shift(flac_out_crc16_words(bits.data(), b0, b1), (uint32_t)(body - b1));
    }
    flac_out_put(bits.data(), FLAC_OUT_SLOT_WORDS, 8u * (uint32_t)body, crc, 16);
    std::vector<uint8_t> out((size_t)body + 2);
    for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)(bits[i >> 2] >> (24 - 8 * (i & 3)));
    return out;
}

static const char* set_text(const std::set<int>& s, std::string* buf) {
    buf->clear();
    for (int v : s) *buf += (buf->empty() ? "" : ",") + std::to_string(v);
    if (buf->empty()) *buf = "-";
    return buf->c_str();
}

int main(int argc, char** argv) {
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        int64_t h[4];
        if (!f || fread(h, 8, 4, f) != 4) {
            fprintf(stderr, "%s: cannot read\n", argv[a]);
            return 2;
        }
        const int channels = (int)h[0], sample_rate = (int)h[1];
        const int64_t frames = h[2];
        std::vector<int16_t> pcm((size_t)(frames * channels));
        std::vector<uint8_t> expected((size_t)h[3]);
        const bool ok = fread(pcm.data(), 2, pcm.size(), f) == pcm.size() && fread(expected.data(), 1, expected.size(), f) == expected.size();
        fclose(f);
        if (!ok || expected.size() < 42) {
            fprintf(stderr, "%s: short case file\n", argv[a]);
            return 2;
        }
        const FlacOutPlan plan = plan_flac_out(1, frames, channels);
        std::vector<uint8_t> file(42);
        Choices ch;
        uint32_t mn = 0xFFFFFF, mx = 0;
        const int64_t blocks = (frames + FLAC_OUT_BLOCK - 1) / FLAC_OUT_BLOCK;
        if (frames > 0 && (plan.refusal || plan.blocks != blocks)) {
            fprintf(stderr, "%s: plan\n", argv[a]);
            return 2;
        }
        for (int64_t b = 0; b < blocks; ++b) {
            const int64_t first = b * FLAC_OUT_BLOCK;
            const int n = (int)(frames - first < FLAC_OUT_BLOCK ? frames - first : FLAC_OUT_BLOCK);
            const std::vector<uint8_t> fr = encode_frame(pcm.data() + first * channels, n, channels, sample_rate, (uint64_t)b, &ch);
            if ((int)fr.size() > plan.slot_stride) fprintf(stderr, "%s: frame %lld outgrows its slot\n", argv[a], (long long)b);
            mn = fr.size() < mn ? (uint32_t)fr.size() : mn, mx = fr.size() > mx ? (uint32_t)fr.size() : mx;
            file.insert(file.end(), fr.begin(), fr.end());
        }
        if (blocks == 0) mn = 0;
        flac_out_streaminfo(file.data(), frames, channels, sample_rate, mn, mx, expected.data() + 26);
        if ((long long)file.size() > flac_out_bound(frames, channels)) fprintf(stderr, "%s: the stream outgrows its bound\n", argv[a]);
        std::string t0, t1, t2, t3;
        if (file == expected) {
            printf("%s: equal frames=%lld assign=%s types=%s orders=%s porders=%s kmax=%d run=%u numbytes=%d\n", argv[a], (long long)blocks, set_text(ch.assign, &t0),
                   set_text(ch.types, &t1), set_text(ch.orders, &t2), set_text(ch.porders, &t3), ch.kmax, ch.run, ch.numbytes);
        } else {
            size_t at = 0;
            while (at < file.size() && at < expected.size() && file[at] == expected[at]) ++at;
            printf("%s: DIFFERENT at byte %zu (%zu bytes, expected %zu)\n", argv[a], at, file.size(), expected.size());
            ++bad;
        }
    }
    return bad ? 1 : 0;
}
