// lm_plan_sweep.cpp - stand-alone host program over csrc/lm_plan.h (tests/test_lm_cpu.py builds it with the host sanitizers): for every
// cache length 1 .. max_len the chunks of plan_lm_decode tile [0, len) exactly once and in order, the split count is what the length
// alone gives, and everything stays inside the bounds lm.hip's scratch is sized for.  Prints one line per regime change:
//   regime <first length> <chunk> <splits at that length>
// and "ok <lengths checked>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../ace-step-1.5-for-windows_amd/csrc/lm_plan.h"

using namespace ace355;

static int fail(int len, const char* what) {
    std::fprintf(stderr, "length %d: %s\n", len, what);
    return 1;
}

int main(int argc, char** argv) {
    const int max_len = argc > 1 ? std::atoi(argv[1]) : 4100;
    if (max_len < 1 || max_len > LM_MAX_POSITIONS) return fail(max_len, "max_len outside 1 .. LM_MAX_POSITIONS");
    int prev_chunk = 0;
    for (int len = 1; len <= max_len; ++len) {
        const LmDecodePlan p = plan_lm_decode(len), again = plan_lm_decode(len);
        if (p.chunk != again.chunk || p.splits != again.splits) return fail(len, "two calls disagree");
        if (p.chunk <= 0 || p.chunk % LM_DECODE_KEY_GROUPS) return fail(len, "chunk is no positive multiple of the key groups");
        if (p.splits < 1 || p.splits > LM_MAX_SPLITS) return fail(len, "split count outside 1 .. LM_MAX_SPLITS");
        if (p.splits != (len + p.chunk - 1) / p.chunk) return fail(len, "split count is not ceil(len / chunk)");
        // the kernel's chunk c = [c * chunk, min(len, (c + 1) * chunk)): every key once, in order, no empty chunk
        std::vector<int> seen(len, 0);
        int next = 0;
        for (int c = 0; c < p.splits; ++c) {
            const int lo = c * p.chunk, hi = lo + p.chunk < len ? lo + p.chunk : len;
            if (lo != next || hi <= lo) return fail(len, "chunks out of order or empty");
            for (int k = lo; k < hi; ++k) ++seen[k];
            next = hi;
        }
        if (next != len) return fail(len, "chunks do not end at len");
        for (int k = 0; k < len; ++k)
            if (seen[k] != 1) return fail(len, "a key is not covered exactly once");
        if (p.chunk != prev_chunk) std::printf("regime %d %d %d\n", len, p.chunk, p.splits);
        prev_chunk = p.chunk;
    }
    // the last regime reaches the longest cache a handle may hold
    const LmDecodePlan top = plan_lm_decode(LM_MAX_POSITIONS);
    if (top.splits > LM_MAX_SPLITS) return fail(LM_MAX_POSITIONS, "split count beyond LM_MAX_SPLITS");
    std::printf("ok %d\n", max_len);
    return 0;
}
