// vae_plan_sweep.cpp - plan_conv / plan_vae / plan_vae_windows (csrc/vae_plan.h) as a stand-alone host program, for a build under
// AddressSanitizer and UBSan (tests/test_vae_plan_cpu.py builds and runs it; it is never loaded into python and needs no GPU).
//   vae_plan_sweep CALLS N
// CALLS lists the conv requests of tests/vae_plan_table.json with their plans and its VAE calls with their step counts and buffer sizes
// (test_vae_plan_cpu.py writes it); each must come out as the file says under the default switches.  Then the grid of requests whose
// conditions vae_plan.h states, under every switch setting, and N seeded random VAE calls on random configurations, lengths, windows,
// budgets and switches.  Every step list is walked the way vae.hip's executor walks it, on buffers of exactly the plan's size: every
// element a step may write is written, so an extent outside its buffer is a sanitizer report.
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <random>
#include <sstream>
#include <string>

#include "../ace-step-1.5-for-windows_amd/csrc/vae_plan.h"

using namespace ace355;

#define REQUIRE(c)                                                              \
    do {                                                                        \
        if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); exit(1); }  \
    } while (0)

static long g_forms[4];   // n32, w4, w8, f8

// The conditions vae_plan.h states about a conv plan
static void check_conv(const ConvRequest& r, const ConvKnobs& kn, const ConvPlan& p) {
    REQUIRE((p.bn == 32 && p.tm == 128 && !p.ws) || (p.bn == 128 && (p.tm == 128 || (p.tm == 256 && (p.ws == 0 || p.ws == 1)))));
    REQUIRE(p.threads == 2 * p.tm && p.grid_z == r.B);
    REQUIRE((p.bn == 32) == (r.N < 128));
    const long tiles_m = (r.M + p.tm - 1) / p.tm, tiles_n = p.ws ? 1 : (r.N + p.bn - 1) / p.bn;
    if (p.ras_tn) {
        REQUIRE(p.ras_tm == tiles_m && p.ras_tn == tiles_n && p.ras_tn > 1 && !p.ws && kn.ras && p.grid_y == 1 && p.grid_x == tiles_m * tiles_n);
    } else {
        REQUIRE(p.ras_tm == 0 && p.grid_x == tiles_m && p.grid_y == tiles_n);
        REQUIRE(!kn.ras || tiles_n == 1 || p.bn == 32 || tiles_m * tiles_n >= (1L << 31));
    }
    REQUIRE((long)p.grid_x * p.tm >= r.M && tiles_n * p.bn >= r.N);   // the grid covers M x N x B
    REQUIRE(!p.ws || r.fused);
    REQUIRE(!r.fused || (p.bn == 128 && (p.tm == 128 || p.ws)));      // a fused unit is never on the 32-column or the plain tall tile
    REQUIRE(!(p.tm == 256 && !p.ws) || (!r.fused && !r.res));         // nor a residual on the tall tile, whatever the switches
    g_forms[p.bn == 32 ? 0 : p.ws ? 3 : p.tm == 256 ? 2 : 1]++;
}

// Walk a step list like the executor: roles to buffers of the plan's size, every writable element written
static void walk(const VaeShape& sh, bool enc, int B, long T, const VaePlan& p, const ConvKnobs& kn) {
    REQUIRE(!p.error && !p.steps.empty() && p.slot_elems > 0);
    std::vector<char> slot[3];
    for (auto& s : slot) s.assign((size_t)p.slot_elems, 0);
    bool written[5] = {false, false, false, true, false};
    size_t n_stage = 1;
    for (const VaeStep& st : p.steps) {
        REQUIRE(st.src >= 0 && st.src <= ACE355_VAE_BUF_IN && written[st.src] && st.dst >= 0 && st.dst <= ACE355_VAE_BUF_OUT && st.dst != ACE355_VAE_BUF_IN);
        REQUIRE(st.res == ACE355_VAE_BUF_NONE || (st.res >= 0 && st.res <= 2 && written[st.res]));
        REQUIRE(st.Cin % 64 == 0 && st.taps >= 1 && (st.taps - 1) * st.dil <= 64 && st.M > 0 && st.N > 0);
        REQUIRE(st.x_valid ? (st.x_shift % 8 == 0 && st.x_valid % 8 == 0) : st.x_shift == 0);
        REQUIRE(!st.fused || (st.Cin == 128 && st.N == 128 && st.taps == 7 && !st.x_valid && st.out_mode == 0));
        REQUIRE(!st.out_snake || st.out_mode == 0);
        if (st.src <= 2) REQUIRE((st.x_valid ? st.x_valid : (long)st.L_in * st.Cin) <= p.slot_elems);
        if (st.dst <= 2) {
            REQUIRE(st.out_mode == 0 && st.y_valid > 0 && st.y_batch_stride == st.y_valid);
            for (long m = 0; m < st.M; m += std::max(1, st.M / 7))   // first, last and a few rows between
                for (long n = 0; n < st.N; ++n) {
                    const long flat = m * st.N + n + st.y_shift;
                    if (flat >= 0 && flat < st.y_valid) slot[st.dst][(size_t)flat] = 1;
                }
            const long last = (long)(st.M - 1) * st.N + st.N - 1 + st.y_shift;
            slot[st.dst][(size_t)std::min(last, (long)st.y_valid - 1)] = 1;
        } else {
            REQUIRE(st.out_mode == 1 && &st == &p.steps.back());
            // (an odd stride's transposed conv gives s L - 1 rows: the window's last core samples do not exist and the kernel's m < M guard drops them)
            bool even = true;
            for (int i = 0; i < sh.nb; ++i) even = even && sh.dec[i].stride % 2 == 0;
            if (!enc) REQUIRE(st.ncl_ld == (long)sh.hop * T && st.ncl_m_lo >= 0 && (st.ncl_m_hi <= st.M || !even) && st.ncl_off + (st.ncl_m_hi - st.ncl_m_lo) <= st.ncl_ld);
        }
        written[st.dst] = true;
        if (st.stage >= 0) {
            REQUIRE((size_t)st.stage == n_stage && n_stage < p.stages.size());
            ++n_stage;
        }
        const ConvRequest rq{B, st.M, st.N, st.Cin, st.taps, st.in_snake != 0, st.x_valid != 0, st.res >= 0, st.fused, 0};
        check_conv(rq, kn, st.plan);
    }
    REQUIRE(n_stage == p.stages.size());
}

static ace355_vae_config config(int dc, int zc, int audio, const std::vector<int>& cm, const std::vector<int>& ups) {
    ace355_vae_config c{};
    c.decoder_channels = dc, c.decoder_input_channels = zc, c.audio_channels = audio, c.num_blocks = (int)cm.size();
    for (size_t i = 0; i < cm.size(); ++i) c.channel_multiples[i] = cm[i], c.upsampling_ratios[i] = ups[i];
    return c;
}

int main(int argc, char** argv) {
    REQUIRE(argc == 3);
    std::ifstream in(argv[1]);
    REQUIRE(in.good());
    const ConvKnobs dflt = CONV_KNOBS_DEFAULT;
    int listed = 0;
    for (std::string line; std::getline(in, line);) {
        std::istringstream ss(line);
        char tag;
        ss >> tag;
        if (tag == 'C') {
            ConvRequest r{};
            ConvPlan w{};
            ss >> r.B >> r.M >> r.N >> r.Cin >> r.taps >> r.in_snake >> r.x_view >> r.res >> r.fused;
            ss >> w.bn >> w.tm >> w.ws >> w.grid_x >> w.grid_y >> w.grid_z >> w.threads >> w.ras_tm >> w.ras_tn;
            REQUIRE(!ss.fail());
            const ConvPlan p = plan_conv(r, dflt);
            check_conv(r, dflt, p);
            REQUIRE(p.bn == w.bn && p.tm == w.tm && p.ws == w.ws && p.grid_x == w.grid_x && p.grid_y == w.grid_y && p.grid_z == w.grid_z &&
                    p.threads == w.threads && p.ras_tm == w.ras_tm && p.ras_tn == w.ras_tn);
        } else if (tag == 'V') {
            int dc, zc, audio, nb, enc, B, n_steps;
            long T, slot;
            ss >> dc >> zc >> audio >> nb;
            std::vector<int> cm(nb), ups(nb);
            for (int& v : cm) ss >> v;
            for (int& v : ups) ss >> v;
            ss >> enc >> B >> T >> n_steps >> slot;
            REQUIRE(!ss.fail());
            const ace355_vae_config c = config(dc, zc, audio, cm, ups);
            REQUIRE(!vae_config_error(c));
            const VaeShape sh = vae_shape(c);
            const VaePlan p = plan_vae(sh, enc != 0, B, T, VaeWindow{0, (int)T, 0, (int)T}, dflt);
            walk(sh, enc != 0, B, T, p, dflt);
            REQUIRE((int)p.steps.size() == n_steps && p.slot_elems == slot);
        } else
            continue;
        ++listed;
    }
    printf("%d listed rows as expected\n", listed);

    // the grid of requests: B 1 .. 8, M around every multiple of 128 up to 4300 and the metric lengths, the widths, taps, the four bits
    const ConvKnobs settings[] = {dflt, {0, 0, 0, -1, 1, 1}, {1, 0, 128, -1, 1, 1}, {1, 0, 256, -1, 1, 1}, {1, 0, 0, 0, 1, 1}, {1, 0, 0, 1, 1, 1},
                                  {1, 0, 0, -1, 0, 1}, {1, 0, 0, -1, 1, 0}, {1, 1, 0, -1, 1, 1}, {1, 0, 0, -1, 0, 0}};
    std::vector<int> Ms = {1, 750, 7500, 45000, 180000, 1440000, 1440001};
    for (int e = 128; e <= 4300; e += 128)
        for (int d = -1; d <= 1; ++d) Ms.push_back(e + d);
    const int Ns[] = {2, 64, 128, 256, 512, 1024, 2048, 1280, 3072, 10240}, Cins[] = {64, 128, 256, 512, 1024, 2048}, tapss[] = {1, 2, 3, 7};
    long grid = 0;
    for (const ConvKnobs& kn : settings)
        for (int B = 1; B <= 8; ++B)
            for (int M : Ms)
                for (int N : Ns)
                    for (int Cin : Cins)
                        for (int taps : tapss)
                            for (int bits = 0; bits < 16; ++bits) {
                                const ConvRequest r{B, M, N, Cin, taps, bits & 1, (bits >> 1) & 1, (bits >> 2) & 1, (bits >> 3) & 1, 0};
                                if (r.fused && !(Cin == 128 && N == 128 && taps == 7 && !r.x_view && r.res)) continue;   // (launch_conv refuses it)
                                const ConvPlan p = plan_conv(r, kn);
                                check_conv(r, kn, p);
                                // each switch moves only what it names
                                const ConvPlan d = plan_conv(r, dflt);
                                if (kn.tm == 256) REQUIRE((r.fused || r.res || p.bn == 32) ? (p.tm == d.tm && p.ws == d.ws) : p.tm == 256);
                                if (kn.tm == 128) REQUIRE(p.ws ? d.ws == 1 : p.tm == 128);
                                if (kn.f8 >= 0) REQUIRE(r.fused ? p.ws == kn.f8 : (p.bn == d.bn && p.tm == d.tm && p.ws == 0 && p.grid_x == d.grid_x));
                                if (!kn.ras) REQUIRE(p.ras_tn == 0 && p.bn == d.bn && p.tm == d.tm && p.ws == d.ws);
                                ++grid;
                            }
    printf("%ld grid requests; forms n32 %ld w4 %ld w8 %ld f8 %ld\n", grid, g_forms[0], g_forms[1], g_forms[2], g_forms[3]);

    // random VAE calls
    const long n_random = atol(argv[2]);
    std::mt19937 rng(355);
    auto pick = [&](int lo, int hi) { return (int)(lo + rng() % (unsigned)(hi - lo + 1)); };
    for (long it = 0; it < n_random; ++it) {
        const int nb = pick(1, 4);
        std::vector<int> cm(nb), ups(nb);
        for (int i = 0; i < nb; ++i) cm[i] = std::min(16, pick(1, 3) * (i ? cm[i - 1] : 1)), ups[i] = pick(2, 5);
        const ace355_vae_config c = config(64 * pick(1, 2), 64, pick(1, 2), cm, ups);
        REQUIRE(!vae_config_error(c));
        const VaeShape sh = vae_shape(c);
        static const int heights[3] = {0, 128, 256};
        const ConvKnobs kn{pick(0, 1), 0, heights[pick(0, 2)], pick(-1, 1), pick(0, 1), pick(0, 1)};
        const int B = pick(1, 5), T = pick(1, 120);
        // the decode under a random budget: the windows tile [0, T), halos cover the receptive field, bytes stay within the budget
        const size_t whole = vae_decode_bytes(sh, B, T);
        const size_t budget = whole / (size_t)pick(1, 12) + 1;
        const VaeWindowPlan wp = plan_vae_windows(sh, B, T, budget, pick(0, 3) ? 0 : 8 * pick(1, 12));
        if (!wp.error) {
            REQUIRE(wp.nb >= 1 && wp.nb <= B && wp.tc >= 1 && wp.tc <= T && wp.ov >= vae_receptive_frames(sh));
            REQUIRE(wp.tc == T || wp.tc % 8 == 0);
            // (the bytes per frame are taken from a 1024-frame window WITH the three buffers' 256-byte tails, so a shorter window's estimate
            //  lacks up to those 768 bytes: the plan may exceed the budget by less than that, never by more)
            REQUIRE(vae_decode_bytes(sh, wp.nb, vae_window_frames(wp, T)) < budget + 768);
            int next = 0;
            for (int cs = 0; cs < T; cs += wp.tc) {
                const VaeWindow w = vae_window_at(wp, T, cs);
                REQUIRE(w.cs == next && w.ce > w.cs && w.ws <= w.cs && w.we >= w.ce && w.ws >= 0 && w.we <= T && w.we - w.ws <= vae_window_frames(wp, T));
                REQUIRE((w.ws == 0 || w.cs - w.ws == wp.ov) && (w.we == T || w.we - w.ce == wp.ov));
                next = w.ce;
                const VaePlan p = plan_vae(sh, false, wp.nb, T, w, kn);
                walk(sh, false, wp.nb, T, p, kn);
                REQUIRE((size_t)p.slot_elems == vae_decode_elems(sh, w.we - w.ws));
            }
            REQUIRE(next == T);
        }
        // the encode: hop * n samples give n frames; any length either plans or is refused as too short
        const long L = (long)sh.hop * pick(1, 40) + (pick(0, 1) ? 0 : pick(0, sh.hop));
        const VaePlan p = plan_vae(sh, true, B, L, VaeWindow{}, kn);
        REQUIRE((p.error != nullptr) == (vae_latent_frames(sh, L) < 0));
        if (!p.error) {
            walk(sh, true, B, L, p, kn);
            REQUIRE(p.out_len == vae_latent_frames(sh, L) && (L % sh.hop || p.out_len == L / sh.hop));
            const int nbg = vae_encode_group(B, L, p.slot_elems, budget);
            REQUIRE(nbg >= 1 && nbg <= B);
        }
    }
    printf("%ld random calls\n", n_random);
    return 0;
}
