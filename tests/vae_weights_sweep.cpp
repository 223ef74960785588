// vae_weights_sweep.cpp - the VAE's weight table (vae_weight_table, vae_weight_slot, vae_pack_index of csrc/vae_plan.h) as a stand-alone
// host program, for a build under AddressSanitizer and UBSan (tests/test_vae_weights_cpu.py builds and runs it; it is never loaded into
// python and needs no GPU).
//   vae_weights_sweep DECODER_CHANNELS LATENT_CHANNELS AUDIO_CHANNELS BLOCKS MULTIPLE.. UPSAMPLING_RATIO..
// First the pack index on small awkward dimensions of each kind against the four formulas the former pack kernels held (restated here as
// literals), then the table of both halves of that configuration as JSON on stdout, every row found again at its slot.
#include <stdio.h>
#include <stdlib.h>

#include "../ace-step-1.5-for-windows_amd/csrc/vae_plan.h"

using namespace ace355;

#define REQUIRE(c)                                                              \
    do {                                                                        \
        if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); exit(1); }  \
    } while (0)

// One kind on raw dimensions [d0][d1][K]: `want(i)` the former kernel's destination of raw element i, (N, taps, Cin) the former builder's
// ConvW, (rows, cols) the former rownorm_kernel arguments.  `holes`: packed elements no raw element lands on.
template <typename F>
static void check_kind(int kind, VaePackDims d, int N, int taps, int Cin, int rows, long cols, long holes, F want) {
    const VaeWeightRow r{"x", kind, d, 1, 0, -1, -1};
    const VaePacked pk = vae_packed(r);
    REQUIRE(pk.N == N && pk.taps == taps && pk.Cin == Cin && pk.elems == (long)N * taps * Cin);
    REQUIRE(vae_norm_rows(r) == rows && vae_norm_cols(r) == cols);
    const long n = (long)d.d0 * d.d1 * d.K;
    REQUIRE(vae_row_tensors(r, true)[0].n == n && vae_row_tensors(r, false)[1].n == rows);
    std::vector<char> hit((size_t)pk.elems, 0);
    for (long i = 0; i < n; ++i) {
        const long j = vae_pack_index(kind, d, i);
        REQUIRE(j >= 0 && j < pk.elems && !hit[(size_t)j] && j == want(i));
        hit[(size_t)j] = 1;
    }
    REQUIRE(pk.elems - n == holes);
}

static void check_pack_index() {
    const int Cout = 3, Cin = 5, K = 7;
    check_kind(VAE_ROW_PLAIN, VaePackDims{Cout, Cin, K, 0}, Cout, K, Cin, Cout, (long)Cin * K, 0, [&](long i) {
        const int k = (int)(i % K);
        const long t = i / K;
        const int ci = (int)(t % Cin), co = (int)(t / Cin);
        return ((long)co * K + k) * Cin + ci;
    });
    for (int s = 1; s <= 3; ++s) {
        const int K2 = 2 * s;
        check_kind(VAE_ROW_CONVT, VaePackDims{Cin, Cout, K2, s}, s * Cout, 2, Cin, Cin, (long)Cout * K2, 0, [&](long i) {
            const int k = (int)(i % K2);
            const long t = i / K2;
            const int co = (int)(t % Cout), ci = (int)(t / Cout);
            const int r = k % s, tap = k >= s ? 0 : 1;
            return (((long)r * Cout + co) * 2 + tap) * Cin + ci;
        });
        check_kind(VAE_ROW_STRIDED, VaePackDims{Cout, Cin, K2, s}, Cout, 2, s * Cin, Cout, (long)Cin * K2, 0, [&](long i) {
            const int k = (int)(i % K2);
            const long t = i / K2;
            const int ci = (int)(t % Cin), co = (int)(t / Cin);
            const int gg = k / s, sp = k % s;
            return ((long)co * 2 + gg) * ((long)s * Cin) + (long)sp * Cin + ci;
        });
    }
    for (int A = 1; A <= 2; ++A) {
        // the former kernel ran over the destination: w'[co][cc] = w[co][c][k] with cc = k * A + c < K * A, zero beyond
        std::vector<long> dst((size_t)Cout * A * K, -1);
        for (long j = 0; j < (long)Cout * 64; ++j) {
            const int cc = (int)(j % 64), co = (int)(j / 64);
            if (cc < K * A) dst[(size_t)(((long)co * A + cc % A) * K + cc / A)] = j;
        }
        check_kind(VAE_ROW_IM2COL, VaePackDims{Cout, A, K, 0}, Cout, 1, 64, Cout, (long)A * K, (long)Cout * (64 - K * A),
                   [&](long i) { return dst[(size_t)i]; });
    }
}

static void print_half(const VaeShape& sh, bool enc) {
    const std::vector<VaeWeightRow> t = vae_weight_table(sh, enc);
    REQUIRE((int)t.size() == 3 + 14 * sh.nb);
    printf("[");
    for (size_t i = 0; i < t.size(); ++i) {
        const VaeWeightRow& r = t[i];
        const bool snake = r.kind == VAE_ROW_SNAKE;
        // the row is at its slot, whatever a step puts into the fields its role does not read
        REQUIRE(vae_weight_slot(sh, enc, snake, r.role, r.block, r.unit) == (int)i);
        if (r.block < 0) REQUIRE(vae_weight_slot(sh, enc, snake, r.role, 3, 2) == (int)i);
        if (r.unit < 0) REQUIRE(vae_weight_slot(sh, enc, snake, r.role, r.block, 2) == (int)i);
        REQUIRE(snake ? (r.bias_reps == 0 && r.d.d1 == 1 && r.d.K == 1 && r.d.s >= 1) : (r.bias_reps == 0 || r.bias_reps == 1 || r.bias_reps == r.d.s));
        const VaePacked pk = snake ? VaePacked{0, 0, 0, 0} : vae_packed(r);
        printf("%s\n  {\"base\": \"%s\", \"kind\": %d, \"d0\": %d, \"d1\": %d, \"K\": %d, \"s\": %d, \"bias_reps\": %d, \"role\": %d, \"block\": %d, \"unit\": %d, "
               "\"norm_rows\": %d, \"norm_cols\": %ld, \"N\": %d, \"taps\": %d, \"Cin\": %d, \"elems\": %ld",
               i ? "," : "", r.base.c_str(), r.kind, r.d.d0, r.d.d1, r.d.K, r.d.s, r.bias_reps, r.role, r.block, r.unit, vae_norm_rows(r),
               vae_norm_cols(r), pk.N, pk.taps, pk.Cin, pk.elems);
        for (int fused = 0; fused < 2; ++fused) {
            printf(", \"%s\": {", fused ? "tensors_fused" : "tensors");
            const std::vector<VaeRawTensor> raw = vae_row_tensors(r, fused != 0);
            for (size_t k = 0; k < raw.size(); ++k) printf("%s\"%s\": %ld", k ? ", " : "", raw[k].name.c_str(), raw[k].n);
            printf("}");
        }
        printf("}");
    }
    printf("]");
}

int main(int argc, char** argv) {
    check_pack_index();
    REQUIRE(argc >= 5);
    ace355_vae_config c{};
    c.decoder_channels = atoi(argv[1]), c.decoder_input_channels = atoi(argv[2]), c.audio_channels = atoi(argv[3]), c.num_blocks = atoi(argv[4]);
    REQUIRE(c.num_blocks >= 1 && c.num_blocks <= ACE355_MAX_BLOCKS && argc == 5 + 2 * c.num_blocks);
    for (int i = 0; i < c.num_blocks; ++i) c.channel_multiples[i] = atoi(argv[5 + i]), c.upsampling_ratios[i] = atoi(argv[5 + c.num_blocks + i]);
    REQUIRE(!vae_config_error(c));
    const VaeShape sh = vae_shape(c);
    printf("{\"decoder\": ");
    print_half(sh, false);
    printf(",\n\"encoder\": ");
    print_half(sh, true);
    printf("}\n");
    return 0;
}
