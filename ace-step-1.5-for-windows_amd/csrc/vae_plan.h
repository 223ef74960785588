// vae_plan.h - the host side of the Oobleck VAE as data, in the shape of attn_plan.h: which conv_kernel instantiation and grid a conv launch
// gets (ConvRequest -> ConvPlan, plan_conv), and the launches of one decode window / one encode group in order (VaeShape -> VaePlan,
// plan_vae) with everything ConvArgs needs except pointers.  launch_conv (conv.hip) executes the first, vae.hip walks the second; the
// public stage list, the buffer sizes, the window plan and the two stage-length recurrences are read off the same data.  The weights of a
// handle are data too (VaeShape -> vae_weight_table): the tensors ace355_vae_finalize asks for, how each is packed (vae_pack_index, shared
// with the pack kernel) and the slot a step's role resolves to (vae_weight_slot).  Pure functions:
// no HIP call, no global, no environment - ace355_conv_plan / ace355_vae_plan answer on a machine without a GPU, and the header compiles
// with a plain host compiler.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/ace355.h"
#include "adapter_plan.h"   // ACE_HD

namespace ace355 {

// Every switch of the conv path, read once per process (conv_knobs, conv.hip).  All are A/B and test hooks.
struct ConvKnobs {
    int ras;        // ACE355_CONV_RAS (1): 0 the plain (m, n, b) grid, 1 XCD-aware rasterisation wherever there is more than one column tile
    int clk;        // ACE355_CONV_CLK (0): ConvArgs::clk_probe, one workgroup records its shader-clock phases and launch_conv prints them
    int tm;         // ACE355_CONV_TM (0): 128 / 256 force the tile height where it is allowed (never the 256-row tile with w2 or a residual)
    int f8;         // ACE355_CONV_F8 (-1): the one-launch residual unit on the 8-wave form 0 never, 1 always; else by problem size
    int fuse_ru;    // ACE355_CONV_FUSE_RU (1): 0 every residual unit as two launches; 1 the C = 128 units as one
    int episnake;   // ACE355_VAE_EPISNAKE (1): the Snake of an activation with ONE reader is applied by its producer's epilogue; 0 by the reader
};
constexpr ConvKnobs CONV_KNOBS_DEFAULT{1, 0, 0, -1, 1, 1};
const ConvKnobs& conv_knobs();

// What the form decision depends on, and nothing else (fields: include/ace355.h).
using ConvRequest = ace355_conv_request;
// conv_kernel<bn, tm, ws> on grid (grid_x, grid_y, grid_z) x threads, ConvArgs::ras_tm / ras_tn.
using ConvPlan = ace355_conv_plan_info;

constexpr int CONV_TALL_K_WGS = 1400, CONV_TALL_T_WGS = 1500;

// Four forms.  <32, 128>: N < 128 (the output conv, the C = 64 units of narrow configurations).  <128, 128>: the 4-wave 128-row tile, the
// default.  <128, 256>: the 8-wave 256-row tile - each weight tile shared by twice the MFMAs, a smaller Snake halo - which wins on every
// k >= 2 launch that fills the chip about one and a half times (512 tall workgroups are resident at once = 1024 four-wave tiles; below
// that the tail of half-empty rounds costs more): k >= 3 convs with Cin >= 128 from 1400 four-wave tiles, the plain-row 2-tap transposed
// convs from 1500 (sweeps: DESIGN 12.9 / 13.7).  It has no registers for residual rows and its fused stage is a form of its own, so a
// launch with a residual or w2 is never tall, also under a forced height (TM=256 on a fused unit once gave a -6 dB decode).  The 2-tap
// convs that stage a Snake or read the strided view stay 4-wave.  <128, 256, 1>: the one-launch unit (C = 128) on 8 waves of 32 rows x 128
// channels, from the same 1400 tiles; its grid is its own (one column tile) and is not rasterised.  Both fused forms give the same bits.
inline ConvPlan plan_conv(const ConvRequest& r, const ConvKnobs& kn) {
    ConvPlan p{};
    p.grid_z = r.B;
    if (r.N < 128) {
        p.bn = 32, p.tm = 128, p.threads = 256;
        p.grid_x = (r.M + 127) / 128, p.grid_y = (r.N + 31) / 32;
        return p;
    }
    const long wgs128 = (long)((r.M + 127) / 128) * ((r.N + 127) / 128) * r.B;
    const bool tall_k = r.Cin >= 128 && r.taps >= 3 && wgs128 >= CONV_TALL_K_WGS;
    const bool tall_t = r.taps == 2 && r.Cin >= 128 && !r.in_snake && !r.x_view && wgs128 >= CONV_TALL_T_WGS;
    const bool tall = !r.fused && !r.res && (kn.tm ? kn.tm == 256 : (tall_k || tall_t));
    p.bn = 128, p.tm = tall ? 256 : 128, p.threads = 2 * p.tm;
    if (r.fused && (kn.f8 >= 0 ? kn.f8 != 0 : wgs128 >= CONV_TALL_K_WGS)) {
        p.tm = 256, p.ws = 1, p.threads = 512;
        p.grid_x = (r.M + 255) / 256, p.grid_y = 1;
        return p;
    }
    p.grid_x = (r.M + p.tm - 1) / p.tm, p.grid_y = (r.N + 127) / 128;
    // Rasterisation: a 1-D grid per item that walks the column tiles of a row block on consecutive slots of one XCD (conv_kernel)
    if (kn.ras && p.grid_y > 1 && (long)p.grid_x * p.grid_y < (1L << 31)) {
        p.ras_tm = p.grid_x, p.ras_tn = p.grid_y;
        p.grid_x *= p.grid_y, p.grid_y = 1;
    }
    return p;
}

// ------------------------------------------------------------------------------------------------ the two halves' shapes
// Widths, strides and pads of both halves, from the configuration alone (ace355_vae_finalize builds its weights from the same numbers:
// vae_weight_table below).
struct VaeBlockShape { int cin, cout, stride, pad; };
struct VaeShape {
    int nb, zc, audio, hop;            // blocks, latent channels, audio channels, product of the strides
    int dec_c0, dec_cl;                // width behind decoder.conv1, width ahead of decoder.conv2
    int eh, enc_cl;                    // encoder width (mean | scale = 2 zc), width ahead of encoder.conv2
    VaeBlockShape dec[ACE355_MAX_BLOCKS], enc[ACE355_MAX_BLOCKS];
};
constexpr int VAE_UNIT_DILS[3] = {1, 3, 9};

// null: a configuration the handle takes; else what ace355_vae_create says about it
inline const char* vae_config_error(const ace355_vae_config& c) {
    if (!(c.num_blocks > 0 && c.num_blocks <= ACE355_MAX_BLOCKS)) return "vae_create: num_blocks";
    if (!(c.decoder_input_channels > 0 && c.decoder_channels > 0 && c.decoder_input_channels % 64 == 0 && c.decoder_channels % 64 == 0))
        return "vae_create: channels must be multiples of 64";
    if (!(c.audio_channels >= 1 && c.audio_channels <= 32)) return "vae_create: audio_channels";
    for (int i = 0; i < c.num_blocks; ++i)
        if (!(c.upsampling_ratios[i] >= 1 && c.channel_multiples[i] >= 1)) return "vae_create: ratios/multiples";
    return nullptr;
}

inline VaeShape vae_shape(const ace355_vae_config& c) {
    VaeShape s{};
    const int nb = s.nb = c.num_blocks;
    s.zc = c.decoder_input_channels, s.audio = c.audio_channels, s.hop = 1, s.eh = 2 * c.decoder_input_channels;
    int cm[ACE355_MAX_BLOCKS + 1];
    cm[0] = 1;
    for (int i = 0; i < nb; ++i) cm[i + 1] = c.channel_multiples[i];
    for (int i = 0; i < nb; ++i) {
        const int up = c.upsampling_ratios[i], down = c.upsampling_ratios[nb - 1 - i];   // downsampling_ratios = reversed upsampling_ratios
        s.hop *= up;
        s.dec[i] = VaeBlockShape{c.decoder_channels * cm[nb - i], c.decoder_channels * cm[nb - i - 1], up, (up + 1) / 2};
        s.enc[i] = VaeBlockShape{s.eh * cm[i], s.eh * cm[i + 1], down, (down + 1) / 2};
    }
    s.dec_c0 = c.decoder_channels * cm[nb], s.dec_cl = c.decoder_channels;
    s.enc_cl = s.eh * cm[nb];
    return s;
}

// The two stage-length recurrences.  ConvTranspose1d(k = 2s, stride s, pad ceil(s / 2)) and Conv1d(k = 2s, stride s, pad ceil(s / 2)).
inline long vae_up_len(long L, const VaeBlockShape& b) { return (L - 1) * b.stride - 2 * b.pad + 2 * b.stride; }
inline long vae_down_len(long L, const VaeBlockShape& b) { return (L + 2 * b.pad - 2 * b.stride) / b.stride + 1; }
// latent frames of an encode of L samples; -1: shorter than one frame
inline long vae_latent_frames(const VaeShape& s, long L) {
    for (int i = 0; i < s.nb && L > 0; ++i) L = vae_down_len(L, s.enc[i]);
    return L > 0 ? L : -1;
}

// ------------------------------------------------------------------------------------------------ the weights of a handle
// One row per conv and per Snake of a half, in state-dict order: what ace355_vae_finalize needs of the loaded tensors, how it packs them,
// and the role a step names the result by.  config.py's weight_shapes() / encoder_weight_shapes() list the same tensors
// (tests/test_vae_weights_cpu.py holds the two against each other).
enum { VAE_ROW_PLAIN = 0, VAE_ROW_CONVT, VAE_ROW_STRIDED, VAE_ROW_IM2COL, VAE_ROW_SNAKE };
constexpr int VAE_IM2COL_COLS = 64;   // virtual channels of the encoder's first conv: K * audio channels, zero-padded
// raw weight(_v) [d0][d1][K]: PLAIN / STRIDED / IM2COL [Cout][Cin][K] (IM2COL: Cin = the audio channels), CONVT [Cin][Cout][K]; K = 2 s
// for the two strided kinds (s = 0 otherwise).  Weight-norm is over dimension 0 for every kind.
struct VaePackDims { int d0, d1, K, s; };
struct VaeWeightRow {
    std::string base;          // "decoder.block.2.res_unit1.conv1"
    int kind;                  // VAE_ROW_*
    VaePackDims d;             // SNAKE: d0 = channels, s = how often the pair is repeated (the strided conv's virtual channels), d1 = K = 1
    int bias_reps;             // 0: no bias; 1: base.bias as loaded; s: repeated s times (one copy per phase filter of CONVT)
    int role, block, unit;     // ACE355_VAE_W_* (ACE355_VAE_SNAKE_* for a SNAKE row) and where, as a step names it
};
struct VaeRawTensor { std::string name; long n; };
struct VaePacked { int N, taps, Cin; long elems; };   // w[N][taps][Cin] as conv_kernel reads it

inline int vae_norm_rows(const VaeWeightRow& r) { return r.d.d0; }
inline long vae_norm_cols(const VaeWeightRow& r) { return (long)r.d.d1 * r.d.K; }
inline VaePacked vae_packed(const VaeWeightRow& r) {
    const VaePackDims& d = r.d;
    VaePacked p = r.kind == VAE_ROW_CONVT     ? VaePacked{d.s * d.d1, 2, d.d0, 0}    // all s phase filters side by side, 2 taps each
                  : r.kind == VAE_ROW_STRIDED ? VaePacked{d.d0, 2, d.s * d.d1, 0}    // 2 taps over s * Cin virtual channels
                  : r.kind == VAE_ROW_IM2COL  ? VaePacked{d.d0, 1, VAE_IM2COL_COLS, 0}
                                              : VaePacked{d.d0, d.K, d.d1, 0};
    p.elems = (long)p.N * p.taps * p.Cin;
    return p;
}
// The tensors a row is built from and their element counts: the weight first.  fused: a pre-fused base.weight stands in for the pair.
inline std::vector<VaeRawTensor> vae_row_tensors(const VaeWeightRow& r, bool fused) {
    if (r.kind == VAE_ROW_SNAKE) return {{r.base + ".alpha", r.d.d0}, {r.base + ".beta", r.d.d0}};
    std::vector<VaeRawTensor> t{{r.base + (fused ? ".weight" : ".weight_v"), vae_norm_rows(r) * vae_norm_cols(r)}};
    if (!fused) t.push_back({r.base + ".weight_g", vae_norm_rows(r)});
    if (r.bias_reps) t.push_back({r.base + ".bias", r.kind == VAE_ROW_CONVT ? r.d.d1 : r.d.d0});
    return t;
}
// Where element i of the raw weight lands in the packed one.  Injective; onto, except that IM2COL leaves columns >= K * d1 of a row (zero).
//   PLAIN    w[co][k][ci]
//   CONVT    w[r * Cout + co][tap][ci], k = r + s <-> tap 0 (x[i0 - 1]), k = r <-> tap 1 (x[i0])
//   STRIDED  w[co][g][s' * Cin + ci], k = g * s + s'
//   IM2COL   w[co][k * A + c]
ACE_HD long vae_pack_index(int kind, const VaePackDims& d, long i) {
    const int k = (int)(i % d.K);
    const long t = i / d.K;
    const int c1 = (int)(t % d.d1), c0 = (int)(t / d.d1);
    switch (kind) {
        case VAE_ROW_CONVT: return (((long)(k % d.s) * d.d1 + c1) * 2 + (k >= d.s ? 0 : 1)) * d.d0 + c0;
        case VAE_ROW_STRIDED: return ((long)c0 * 2 + k / d.s) * ((long)d.s * d.d1) + (long)(k % d.s) * d.d1 + c1;
        case VAE_ROW_IM2COL: return (long)c0 * VAE_IM2COL_COLS + k * d.d1 + c1;
        default: return ((long)c0 * d.K + k) * d.d1 + c1;
    }
}

// Position in vae_weight_table(sh, enc) of the row a step names: conv1, 14 rows per block, the final Snake, conv2.  -1: no such role.
inline int vae_weight_slot(const VaeShape& sh, bool enc, bool snake, int role, int block, int unit) {
    const int b0 = 1 + 14 * block, u0 = b0 + (enc ? 0 : 2) + 4 * unit, end = 1 + 14 * sh.nb;
    if (snake) switch (role) {
        case ACE355_VAE_SNAKE_UNIT_S1: return u0;
        case ACE355_VAE_SNAKE_UNIT_S2: return u0 + 2;
        case ACE355_VAE_SNAKE_BLOCK: return b0 + (enc ? 12 : 0);
        case ACE355_VAE_SNAKE_FINAL: return end;
        default: return -1;
    }
    switch (role) {
        case ACE355_VAE_W_CONV_IN: return 0;
        case ACE355_VAE_W_CONVT: return enc ? -1 : b0 + 1;
        case ACE355_VAE_W_UNIT_C1: return u0 + 1;
        case ACE355_VAE_W_UNIT_C2: return u0 + 3;
        case ACE355_VAE_W_DOWN: return enc ? b0 + 13 : -1;
        case ACE355_VAE_W_OUT: return enc ? -1 : end + 1;
        case ACE355_VAE_W_HEAD: return enc ? end + 1 : -1;
        default: return -1;
    }
}

inline std::vector<VaeWeightRow> vae_weight_table(const VaeShape& sh, bool enc) {
    std::vector<VaeWeightRow> t;
    t.reserve(3 + 14 * sh.nb);
    auto conv = [&](const std::string& base, int kind, int d0, int d1, int K, int s, int bias_reps, int role, int block, int unit) {
        t.push_back(VaeWeightRow{base, kind, VaePackDims{d0, d1, K, s}, bias_reps, role, block, unit});
    };
    auto snake = [&](const std::string& base, int C, int reps, int role, int block, int unit) {
        t.push_back(VaeWeightRow{base, VAE_ROW_SNAKE, VaePackDims{C, 1, 1, reps}, 0, role, block, unit});
    };
    auto unit = [&](const std::string& p, int b, int j, int C) {
        const std::string r = p + ".res_unit" + std::to_string(j + 1);
        snake(r + ".snake1", C, 1, ACE355_VAE_SNAKE_UNIT_S1, b, j);
        conv(r + ".conv1", VAE_ROW_PLAIN, C, C, 7, 0, 1, ACE355_VAE_W_UNIT_C1, b, j);
        snake(r + ".snake2", C, 1, ACE355_VAE_SNAKE_UNIT_S2, b, j);
        conv(r + ".conv2", VAE_ROW_PLAIN, C, C, 1, 0, 1, ACE355_VAE_W_UNIT_C2, b, j);
    };
    if (!enc) {
        conv("decoder.conv1", VAE_ROW_PLAIN, sh.dec_c0, sh.zc, 7, 0, 1, ACE355_VAE_W_CONV_IN, -1, -1);
        for (int i = 0; i < sh.nb; ++i) {
            const VaeBlockShape& S = sh.dec[i];
            const std::string p = "decoder.block." + std::to_string(i);
            snake(p + ".snake1", S.cin, 1, ACE355_VAE_SNAKE_BLOCK, i, -1);
            conv(p + ".conv_t1", VAE_ROW_CONVT, S.cin, S.cout, 2 * S.stride, S.stride, S.stride, ACE355_VAE_W_CONVT, i, -1);
            for (int j = 0; j < 3; ++j) unit(p, i, j, S.cout);
        }
        snake("decoder.snake1", sh.dec_cl, 1, ACE355_VAE_SNAKE_FINAL, -1, -1);
        conv("decoder.conv2", VAE_ROW_PLAIN, sh.audio, sh.dec_cl, 7, 0, 0, ACE355_VAE_W_OUT, -1, -1);
        return t;
    }
    // vae_model.py:148-187.  encoder_hidden_size = 2 * latent channels (mean | scale)
    conv("encoder.conv1", VAE_ROW_IM2COL, sh.eh, sh.audio, 7, 0, 1, ACE355_VAE_W_CONV_IN, -1, -1);
    for (int i = 0; i < sh.nb; ++i) {
        const VaeBlockShape& S = sh.enc[i];
        const std::string p = "encoder.block." + std::to_string(i);
        for (int j = 0; j < 3; ++j) unit(p, i, j, S.cin);
        snake(p + ".snake1", S.cin, S.stride, ACE355_VAE_SNAKE_BLOCK, i, -1);
        conv(p + ".conv1", VAE_ROW_STRIDED, S.cout, S.cin, 2 * S.stride, S.stride, 1, ACE355_VAE_W_DOWN, i, -1);
    }
    snake("encoder.snake1", sh.enc_cl, 1, ACE355_VAE_SNAKE_FINAL, -1, -1);
    conv("encoder.conv2", VAE_ROW_PLAIN, sh.eh, sh.enc_cl, 3, 0, 1, ACE355_VAE_W_HEAD, -1, -1);
    return t;
}

// ------------------------------------------------------------------------------------------------ one window / one group as steps
using VaeStep = ace355_vae_step_info;
// latent frames [ws, we) of every item are decoded (rows outside are zero: the true padding at the sequence ends, discarded halo
// elsewhere), the samples of frames [cs, ce) are written.  The encoder has no windows.
struct VaeWindow { int ws, we, cs, ce; };

struct VaePlan {
    const char* error = nullptr;                   // "audio shorter than one latent frame" (encoder); the vectors are then unfinished
    std::vector<VaeStep> steps;                    // launch order
    std::vector<ace355_vae_stage_info> stages;     // the stored tensors (ACE355_VAE_STAGE_*): [0] is the input image, then one per step with stage >= 0
    long slot_elems = 0;                           // per item: the largest extent a step writes to a ping-pong slot
    long out_len = 0;                              // per item: samples of the window (decoder) / latent frames (encoder)
};

// Residual unit: x + conv_k1(snake2(conv_k7_dil(snake1(x)))), in place on the block state with one scratch slot.  At C = 128 one workgroup
// tile spans all channels and the k = 1 conv runs on the k = 7 result inside the same launch (ConvArgs::w2); the output then lands in the
// scratch slot (neighbouring tiles still read the state's halo rows) and the two slots trade places.  With kn.episnake a Snake whose
// input has ONE reader is applied by that input's producer (ConvArgs::osnake_a), once per element and from the fp32 sum: snake2 by an
// unfused unit's k = 7 conv, a block's first Snake (or the final one) by whatever launch precedes it.
inline VaePlan plan_vae(const VaeShape& sh, bool enc, int B, long T, const VaeWindow& win, const ConvKnobs& kn) {
    VaePlan p;
    p.steps.reserve(2 + 7 * sh.nb);
    p.stages.reserve(3 + 7 * sh.nb);
    const bool epi = kn.episnake != 0 && (enc || sh.nb > 0);
    int slot_stage[5] = {-1, -1, -1, 0, -1};   // the stage each buffer holds
    auto stage = [&](int kind, int block, int unit, int channels, int flags, int src, int res, int dil, long rows) {
        p.stages.push_back(ace355_vae_stage_info{kind, block, unit, channels, flags, src, res, dil, rows});
    };
    // One launch.  `kind` < 0: no public stage.  Flags, sources and rows of the stage follow from the step.
    auto conv = [&](VaeStep st, int kind, int channels, long rows) {
        st.plan = plan_conv(ConvRequest{B, st.M, st.N, st.Cin, st.taps, st.in_snake != 0, st.x_valid != 0, st.res >= 0, st.fused, 0}, kn);
        st.stage = -1;
        if (kind >= 0) {
            const int flags = (st.in_snake ? ACE355_VAE_FLAG_IN_SNAKE : 0) | (st.out_snake ? ACE355_VAE_FLAG_OUT_SNAKE : 0) |
                              (st.fused ? ACE355_VAE_FLAG_FUSED : 0) | (st.out_mode ? ACE355_VAE_FLAG_F32_NCL : 0);
            st.stage = (int)p.stages.size();
            stage(kind, st.block, st.unit, channels, flags, slot_stage[st.src], st.res >= 0 ? slot_stage[st.res] : -1, st.dil, rows);
            st.stage_info = p.stages.back();
            slot_stage[st.dst] = st.stage;
        }
        if (st.dst <= ACE355_VAE_BUF_SLOT0 + 2) p.slot_elems = std::max(p.slot_elems, (long)st.y_valid);
        p.steps.push_back(st);
    };
    // a plain stride-1 conv over L rows: Cin -> N channels, bf16 rows out
    auto plain = [](int weight, int block, int unit, int src, int dst, long L, int Cin, int N, int taps, int dil) {
        VaeStep st{};
        st.weight = weight, st.block = block, st.unit = unit, st.src = src, st.dst = dst, st.res = ACE355_VAE_BUF_NONE;
        st.Cin = Cin, st.N = N, st.taps = taps, st.dil = dil, st.center = taps / 2, st.L_in = (int)L, st.M = (int)L;
        st.x_batch_stride = L * Cin, st.y_batch_stride = st.y_valid = L * N;
        return st;
    };
    auto unit = [&](int block, int j, int& state, int& tmp, long L, int C, int out_snake, int out_snake_block) {
        VaeStep k7 = plain(ACE355_VAE_W_UNIT_C1, block, j, state, tmp, L, C, C, 7, VAE_UNIT_DILS[j]);
        k7.in_snake = ACE355_VAE_SNAKE_UNIT_S1, k7.in_snake_block = block;
        if (kn.fuse_ru && C == 128) {
            k7.fused = 1, k7.res = state, k7.res_batch_stride = L * C;
            k7.out_snake = out_snake, k7.out_snake_block = out_snake_block;
            conv(k7, ACE355_VAE_STAGE_UNIT, C, L);
            std::swap(state, tmp);
            return;
        }
        if (epi) k7.out_snake = ACE355_VAE_SNAKE_UNIT_S2, k7.out_snake_block = block;   // its only reader is the k = 1 conv below
        conv(k7, ACE355_VAE_STAGE_UNIT_K7, C, L);
        VaeStep k1 = plain(ACE355_VAE_W_UNIT_C2, block, j, tmp, state, L, C, C, 1, 1);
        if (!epi) k1.in_snake = ACE355_VAE_SNAKE_UNIT_S2, k1.in_snake_block = block;
        k1.out_snake = out_snake, k1.out_snake_block = out_snake_block;
        k1.res = state, k1.res_batch_stride = L * C;
        conv(k1, ACE355_VAE_STAGE_UNIT_K1, C, L);
    };
    int cur = 0, nxt = 1, tmp = 2;
    if (!enc) {
        long L = win.we - win.ws;
        stage(ACE355_VAE_STAGE_INPUT, -1, -1, sh.zc, 0, -1, -1, 1, L);
        // conv1: k7, no Snake ahead of it; the window's rows of the whole-sequence latent image
        VaeStep st = plain(ACE355_VAE_W_CONV_IN, -1, -1, ACE355_VAE_BUF_IN, cur, L, sh.zc, sh.dec_c0, 7, 1);
        st.src_off = (long)win.ws * sh.zc, st.x_batch_stride = T * sh.zc;
        if (epi) st.out_snake = ACE355_VAE_SNAKE_BLOCK, st.out_snake_block = 0;
        conv(st, ACE355_VAE_STAGE_CONV_IN, sh.dec_c0, L);
        for (int bi = 0; bi < sh.nb; ++bi) {
            const VaeBlockShape& bk = sh.dec[bi];
            const long Lout = vae_up_len(L, bk);
            // Snake -> ConvTranspose1d as the 2-tap polyphase GEMM: N = s * cout (all s phase filters side by side), row i0 is the flat
            // output span [(i0 s - pad) cout, + s cout): a shift of -pad * cout, cropped to the stage
            st = plain(ACE355_VAE_W_CONVT, bi, -1, cur, nxt, L, bk.cin, bk.stride * bk.cout, 2, 1);
            if (!epi) st.in_snake = ACE355_VAE_SNAKE_BLOCK, st.in_snake_block = bi;
            st.M = (int)L + 1, st.center = 1;
            st.y_batch_stride = st.y_valid = Lout * bk.cout, st.y_shift = -(long)bk.pad * bk.cout;
            conv(st, ACE355_VAE_STAGE_CONVT, bk.cout, Lout);
            // the reader of the block's output: the next block's transposed conv, or the output conv
            const bool last = bi + 1 == sh.nb;
            for (int j = 0; j < 3; ++j)
                unit(bi, j, nxt, tmp, Lout, bk.cout, epi && j == 2 ? (last ? ACE355_VAE_SNAKE_FINAL : ACE355_VAE_SNAKE_BLOCK) : 0,
                     epi && j == 2 && !last ? bi + 1 : 0);
            std::swap(cur, nxt);
            L = Lout;
        }
        // Snake -> conv k7 -> f32 [audio][hop T] per item: the window's core samples go straight to their place in the call's output
        const long hop = sh.hop, Lall = hop * T;
        st = plain(ACE355_VAE_W_OUT, -1, -1, cur, ACE355_VAE_BUF_OUT, L, sh.dec_cl, sh.audio, 7, 1);
        if (!epi) st.in_snake = ACE355_VAE_SNAKE_FINAL;
        st.y_batch_stride = Lall * sh.audio, st.y_valid = 0;
        st.out_mode = 1, st.n_real = sh.audio;
        st.ncl_ld = Lall, st.ncl_off = (long)win.cs * hop, st.ncl_m_lo = (int)((win.cs - win.ws) * hop), st.ncl_m_hi = (int)((win.ce - win.ws) * hop);
        conv(st, -1, 0, 0);
        p.out_len = L;
        return p;
    }
    long L = T;
    stage(ACE355_VAE_STAGE_INPUT, -1, -1, 64, 0, -1, -1, 1, L);
    // conv1 (k7 over the audio channels) as one tap over the im2col'ed rows
    conv(plain(ACE355_VAE_W_CONV_IN, -1, -1, ACE355_VAE_BUF_IN, cur, L, 64, sh.eh, 1, 1), ACE355_VAE_STAGE_CONV_IN, sh.eh, L);
    for (int bi = 0; bi < sh.nb; ++bi) {
        const VaeBlockShape& bk = sh.enc[bi];
        for (int j = 0; j < 3; ++j) unit(bi, j, cur, tmp, L, bk.cin, epi && j == 2 ? ACE355_VAE_SNAKE_BLOCK : 0, epi && j == 2 ? bi : 0);
        const long Lo = vae_down_len(L, bk);
        if (Lo <= 0) { p.error = "audio shorter than one latent frame"; return p; }
        // Snake -> Conv1d(k = 2s, stride s) as 2 taps over the shifted view x'[r][c'] = x_flat[(r s - pad) cin + c'] of s * cin virtual channels
        VaeStep st = plain(ACE355_VAE_W_DOWN, bi, -1, cur, nxt, Lo, bk.stride * bk.cin, bk.cout, 2, 1);
        st.L_in = (int)Lo + 1, st.center = 0;
        st.x_batch_stride = st.x_valid = L * bk.cin, st.x_shift = -(long)bk.pad * bk.cin;
        if (!epi) st.in_snake = ACE355_VAE_SNAKE_BLOCK, st.in_snake_block = bi;
        if (epi && bi + 1 == sh.nb) st.out_snake = ACE355_VAE_SNAKE_FINAL;   // read by conv2 only
        conv(st, ACE355_VAE_STAGE_DOWN, bk.cout, Lo);
        std::swap(cur, nxt);
        L = Lo;
    }
    // Snake -> conv k3 -> f32 [2 Z][T] per item, ahead of the diagonal Gaussian head
    VaeStep st = plain(ACE355_VAE_W_HEAD, -1, -1, cur, ACE355_VAE_BUF_OUT, L, sh.enc_cl, sh.eh, 3, 1);
    if (!epi || sh.nb == 0) st.in_snake = ACE355_VAE_SNAKE_FINAL;
    st.y_batch_stride = (long)sh.eh * L, st.y_valid = 0;
    st.out_mode = 1, st.n_real = sh.eh;
    conv(st, ACE355_VAE_STAGE_HEAD, sh.eh, L);
    p.out_len = L;
    return p;
}

// ------------------------------------------------------------------------------------------------ memory: sizes, windows, groups
// Elements per item of each of the three ping-pong buffers for a decode of `frames` latent frames: the largest extent over the steps.
inline size_t vae_decode_elems(const VaeShape& s, long frames) {
    return (size_t)plan_vae(s, false, 1, frames, VaeWindow{0, (int)frames, 0, (int)frames}, CONV_KNOBS_DEFAULT).slot_elems;
}
inline size_t vae_decode_bytes(const VaeShape& s, int nb, long frames) { return 3 * (vae_decode_elems(s, frames) * (size_t)nb * 2 + 256); }

// Receptive half-width of one output sample in LATENT frames: conv1 (k7) + per block {2-tap polyphase transposed conv at the input
// rate, three k7 residual units with dilations 1 / 3 / 9 at the output rate} + the k7 output conv.  Everything further away from a
// window edge than this is bit-identical to the whole-sequence decode (same per-element MFMA accumulation order).
inline int vae_receptive_frames(const VaeShape& s) {
    double rf = 3.0, rate = 1.0;
    for (int i = 0; i < s.nb; ++i) {
        rf += 1.0 / rate;
        rate *= s.dec[i].stride;
        rf += 3.0 * (1 + 3 + 9) / rate;
    }
    rf += 3.0 / rate;
    return (int)ceil(rf);
}

// Window plan of a decode under the activation budget: whole batch and whole sequence when the three ping-pong buffers fit; else fewer
// items per window (exact: items are independent); else windows of `tc` core frames with `ov` halo frames on either side, the halo
// decoded and discarded.  overlap 0: max(16, receptive field + 2 rounded up to 8).
struct VaeWindowPlan { const char* error; int nb, tc, ov; };
inline VaeWindowPlan plan_vae_windows(const VaeShape& s, int B, int T, size_t budget, int overlap) {
    const int rf = vae_receptive_frames(s);
    VaeWindowPlan w{nullptr, B, T, overlap > 0 ? overlap : std::max(16, ((rf + 2 + 7) / 8) * 8)};
    if (w.ov < rf) { w.error = "vae_decode: the window overlap must cover the decoder's receptive field"; return w; }
    if (vae_decode_bytes(s, B, T) <= budget) return w;
    const size_t per_item = vae_decode_bytes(s, 1, T);
    if (per_item <= budget) {
        w.nb = (int)std::max<size_t>(1, std::min<size_t>(B, budget / per_item));
        return w;
    }
    // bytes grow linearly in the window length: largest window that fits, minus the two halos
    const size_t per_frame = vae_decode_bytes(s, 1, 1024) / 1024 + 1;
    const long win = (long)(budget / per_frame);
    w.tc = (int)std::min<long>(T, win - 2L * w.ov);
    if (w.tc < w.ov) { w.error = "vae_decode: the activation budget is smaller than one decode window (raise ACE355_VAE_BUDGET_MB)"; return w; }
    w.tc = (w.tc / 8) * 8;  // (whole 8-frame groups: window starts stay 16-byte aligned in the latent rows)
    // several items per window when they fit
    const size_t per_win = vae_decode_bytes(s, 1, std::min<long>(T, w.tc + 2L * w.ov));
    w.nb = (int)std::max<size_t>(1, std::min<size_t>(B, budget / per_win));
    return w;
}
// frames one window of the plan decodes, halos included
inline long vae_window_frames(const VaeWindowPlan& w, int T) { return std::min<long>(T, w.tc == T ? T : w.tc + 2L * w.ov); }
// window `cs` (its first core frame) of the plan
inline VaeWindow vae_window_at(const VaeWindowPlan& w, int T, int cs) {
    const int ce = std::min(T, cs + w.tc);
    return w.tc == T ? VaeWindow{0, T, cs, ce} : VaeWindow{std::max(0, cs - w.ov), std::min(T, ce + w.ov), cs, ce};
}

// Items per group of an encode of L samples under the same budget (exact: items are independent): three slots plus the im2col image.
inline int vae_encode_group(int B, long L, long slot_elems, size_t budget) {
    const size_t per_item = (size_t)slot_elems * 2 * 3 + (size_t)L * 64 * 2;
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)B, budget / std::max<size_t>(per_item, 1)));
}

}  // namespace ace355
