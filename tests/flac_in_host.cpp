// flac_in_host.cpp - the per-frame routines of csrc/flac_in.h, exactly as the GPU kernels of csrc/flac_in.hip call them, run on the CPU by a
// stand-alone program (tests/test_flac_in_cpu.py builds it with -fsanitize=address,undefined and runs it directly).
//   flac_in_host decode  FILE...      every frame of every case decodes with status ok to the expected samples
//   flac_in_host corrupt N SEED FILE...   N seeded single-bit / single-byte corruptions of the frames, spread over the cases: every frame
//                                     ends with "status != ok, or its samples are the expected ones", and the program prints how many
//                                     frames each status code caught
// A case file (little endian): int64 channels, bps, sample_rate, variable, total, n_frames, max_block, file_bytes; int64 table[n_frames][4]
// (byte offset, byte length, first sample, block); int64 expected[total][channels]; the FLAC file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../ace-step-1.5-for-windows_amd/csrc/flac_in.h"

using namespace ace355;

struct Case {
    std::string name;
    FlacStreamParams sp;
    int64_t total, n_frames, max_block, file_bytes;
    std::vector<int64_t> table, expected;
    std::vector<uint8_t> file;   // allocated to the next multiple of 4, zero padded: what the device buffer is
};

static bool read_case(const char* path, Case* c) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    int64_t h[8];
    bool ok = fread(h, 8, 8, f) == 8;
    if (ok) {
        c->name = path, c->sp = FlacStreamParams{(int32_t)h[0], (int32_t)h[1], (int32_t)h[2], (int32_t)h[3]};
        c->total = h[4], c->n_frames = h[5], c->max_block = h[6], c->file_bytes = h[7];
        c->table.resize((size_t)c->n_frames * 4), c->expected.resize((size_t)(c->total * h[0])), c->file.assign((size_t)((c->file_bytes + 3) / 4 * 4), 0);
        ok = fread(c->table.data(), 8, c->table.size(), f) == c->table.size() && fread(c->expected.data(), 8, c->expected.size(), f) == c->expected.size() &&
             fread(c->file.data(), 1, (size_t)c->file_bytes, f) == (size_t)c->file_bytes;
    }
    fclose(f);
    return ok;
}

// The three passes over one case, frame by frame, with the row checks of flac_in.hip's load_row.  out [total][channels], status [n_frames].
static void decode(const Case& c, const uint8_t* file, std::vector<int32_t>* out, std::vector<int>* status) {
    const int ch = c.sp.channels;
    out->assign((size_t)(c.total * ch), 0), status->assign((size_t)c.n_frames, FLAC_HEADER_MISMATCH);
    for (int64_t f = 0; f < c.n_frames; ++f) {
        const int64_t off = c.table[4 * f], len = c.table[4 * f + 1], first = c.table[4 * f + 2], block = c.table[4 * f + 3];
        if (!(off >= 0 && len >= 0 && off <= c.file_bytes && len <= c.file_bytes - off && block >= 1 && block <= c.max_block && first >= 0 &&
              first <= c.total && block <= c.total - first))
            continue;
        std::vector<int32_t> c0((size_t)block), c1((size_t)block);   // exact sizes: a store outside [0, block) is a sanitizer report
        FlacSubDesc d[2];
        int32_t assign = 0;
        const int st = flac_frame_entropy(file, off, len, c.sp.variable ? (uint64_t)first : (uint64_t)f, (int)block, c.sp, c0.data(), c1.data(), d, &assign);
        (*status)[(size_t)f] = st;
        if (st != FLAC_OK) continue;
        flac_subframe_restore(c0.data(), (int)block, &d[0]);
        if (ch == 2) flac_subframe_restore(c1.data(), (int)block, &d[1]);
        for (int64_t i = 0; i < block; ++i) {
            int32_t l, r;
            flac_finish_sample(c0[(size_t)i], ch == 2 ? c1[(size_t)i] : 0, d[0].wasted, ch == 2 ? d[1].wasted : 0, ch == 2 ? assign : 0, &l, &r);
            (*out)[(size_t)((first + i) * ch)] = l;
            if (ch == 2) (*out)[(size_t)((first + i) * ch + 1)] = r;
        }
    }
}

static bool frame_equal(const Case& c, const std::vector<int32_t>& out, int64_t f) {
    const int ch = c.sp.channels;
    const int64_t first = c.table[4 * f + 2], block = c.table[4 * f + 3];
    for (int64_t i = first * ch; i < (first + block) * ch; ++i)
        if ((int64_t)out[(size_t)i] != c.expected[(size_t)i]) return false;
    return true;
}

static uint64_t rng_state;
static uint64_t rng() {   // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull, z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

int main(int argc, char** argv) {
    if (argc < 3) return fprintf(stderr, "usage: flac_in_host decode FILE... | corrupt N SEED FILE...\n"), 2;
    const bool corrupt = strcmp(argv[1], "corrupt") == 0;
    const int first_file = corrupt ? 4 : 2;
    if (corrupt && argc < 5) return fprintf(stderr, "corrupt needs N SEED FILE...\n"), 2;
    std::vector<Case> cases((size_t)(argc - first_file));
    for (int i = first_file; i < argc; ++i)
        if (!read_case(argv[i], &cases[(size_t)(i - first_file)])) return fprintf(stderr, "cannot read %s\n", argv[i]), 2;
    std::vector<int32_t> out;
    std::vector<int> status;
    if (!corrupt) {
        for (const Case& c : cases) {
            decode(c, c.file.data(), &out, &status);
            for (int64_t f = 0; f < c.n_frames; ++f)
                if (status[(size_t)f] != FLAC_OK || !frame_equal(c, out, f))
                    return fprintf(stderr, "%s: frame %lld status %d, samples %s\n", c.name.c_str(), (long long)f, status[(size_t)f], frame_equal(c, out, f) ? "equal" : "differ"), 1;
            printf("%s: %lld frames, %lld samples x %d channels at %d bits: equal\n", c.name.c_str(), (long long)c.n_frames, (long long)c.total, c.sp.channels, c.sp.bps);
        }
        return 0;
    }
    const long n = atol(argv[2]);
    rng_state = (uint64_t)atoll(argv[3]);
    long caught[6] = {0, 0, 0, 0, 0, 0}, intact = 0, bits = 0, bytes = 0;
    for (long k = 0; k < n; ++k) {
        const Case& c = cases[(size_t)k % cases.size()];
        std::vector<uint8_t> file(c.file);   // (its own exact-size allocation)
        const int64_t lo = c.table[0], at = lo + (int64_t)(rng() % (uint64_t)(c.file_bytes - lo));
        if (k & 1) {
            file[(size_t)at] ^= (uint8_t)(1 + rng() % 255), ++bytes;
        } else {
            file[(size_t)at] ^= (uint8_t)(1u << (rng() % 8)), ++bits;
        }
        decode(c, file.data(), &out, &status);
        for (int64_t f = 0; f < c.n_frames; ++f) {
            const int st = status[(size_t)f];
            if (st != FLAC_OK) ++caught[st < 6 ? st : 0];
            else if (frame_equal(c, out, f)) ++intact;
            else return fprintf(stderr, "%s: corruption %ld at byte %lld: frame %lld reports ok with wrong samples\n", c.name.c_str(), k, (long long)at, (long long)f), 1;
        }
    }
    printf("corruptions %ld (%ld single-bit, %ld single-byte) over %zu streams: frames caught by header mismatch %ld, reserved code %ld, overrun %ld, "
           "sample count %ld, CRC-16 %ld; frames left intact %ld; ok with wrong samples 0\n",
           n, bits, bytes, cases.size(), caught[1], caught[2], caught[3], caught[4], caught[5], intact);
    return 0;
}
