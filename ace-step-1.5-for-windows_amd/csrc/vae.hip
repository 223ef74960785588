// vae.hip - the Oobleck VAE handle behind ace355.h: weight-norm fusion + packing at load time, whole-sequence decode
// (architecture per acestep/models/mlx/vae_model.py:190-230) and - SURVEY.md section 8f row N3 - whole-sequence encode
// (vae_model.py:92-116, 148-187, 285-310) as chains of conv_kernel launches (conv.hip).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "encoder.h"   // LoadBase, dev_alloc
#include "vae_plan.h"

using namespace ace355;

namespace {

struct ConvW {
    bf16_t* w = nullptr;   // [N][taps][Cin]
    float* bias = nullptr; // [N] or null
};
struct SnakeP {
    float* ea = nullptr;  // exp(alpha)
    float* ib = nullptr;  // 1 / (exp(beta) + 1e-9)
};
struct RawT {
    float* p = nullptr;
    long n = 0;
};
// device temporaries of a load or a finalize: freed on every exit path
struct DevTmp {
    std::vector<void*> bag;
    ~DevTmp() { for (void* q : bag) (void)hipFree(q); }
};

// ||v_row||_2 per row (one wave per row)
__global__ void rownorm_kernel(const float* __restrict__ v, long cols, float* __restrict__ out, int rows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    double s = 0;
    for (long c = lane; c < cols; c += 64) {
        const double x = v[(long)row * cols + c];
        s += x * x;
    }
    s = wave_sum_d(s);
    if (lane == 0) out[row] = (float)sqrt(s);
}
// weight(_v) [d0][d1][K] (+ g and the norm over dimension 0) -> bf16 at vae_pack_index (vae_plan.h)
__global__ void pack_weight_kernel(const float* __restrict__ v, const float* __restrict__ g, const float* __restrict__ nrm,
                                   bf16_t* __restrict__ w, int kind, VaePackDims d, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x = v[i];
    if (g) {
        const long r = i / ((long)d.d1 * d.K);
        x = g[r] * x / (nrm[r] + 1e-9f);
    }
    w[vae_pack_index(kind, d, i)] = f2bf(x);
}
// Snake parameters as conv_kernel takes them, the pair of C repeated `reps` times
__global__ void snake_prep_kernel(const float* __restrict__ alpha, const float* __restrict__ beta, float* __restrict__ ea,
                                  float* __restrict__ ib, int C, int reps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C * reps) return;
    ea[i] = expf(alpha[i % C]);
    ib[i] = 1.0f / (expf(beta[i % C]) + 1e-9f);
}
// audio f32 [B][A][L] -> x'[b][l][k*A + c] = audio[b][c][l + k - K/2] (zero outside), 64 bf16 per row
__global__ void audio_im2col_kernel(const float* __restrict__ audio, bf16_t* __restrict__ out, int A, long L, int K, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cc = (int)(i % 64);
    const long bl = i / 64;
    const long l = bl % L, b = bl / L;
    float x = 0.f;
    if (cc < K * A) {
        const int k = cc / A, c = cc % A;
        const long src = l + k - K / 2;
        if (src >= 0 && src < L) x = audio[(b * A + c) * L + src];
    }
    out[i] = f2bf(x);
}
// OobleckDiagonalGaussianDistribution: h f32 [B][2*Z][T] -> z[b][c][t] = mean + (softplus(scale) + 1e-4) * noise (noise null: mean)
__global__ void gaussian_head_kernel(const float* __restrict__ h, const float* __restrict__ noise, float* __restrict__ z, int Z, long T,
                                     long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long t = i % T;
    const long bc = i / T;
    const long c = bc % Z, b = bc / Z;
    const float mean = h[(b * 2 * Z + c) * T + t];
    float out = mean;
    if (noise) {
        const float sc = h[(b * 2 * Z + Z + c) * T + t];
        const float sp = sc > 20.f ? sc : log1pf(expf(sc));
        out = mean + (sp + 1e-4f) * noise[i];
    }
    z[i] = out;
}
__global__ void tile_bias_kernel(const float* __restrict__ b, float* __restrict__ out, int C, int reps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C * reps) return;
    out[i] = b[i % C];
}
__global__ void cvt_bf16_f32_kernel(const bf16_t* __restrict__ in, float* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = bf2f(in[i]);
}

}  // namespace

int ace355::launch_snake_prep(const float* alpha, const float* beta, float* ea, float* ib, int C, int reps, hipStream_t s) {
    hipLaunchKernelGGL(snake_prep_kernel, dim3((C * reps + 255) / 256), dim3(256), 0, s, alpha, beta, ea, ib, C, reps);
    ACE_LAUNCH_CHECK();
    return 0;
}

struct ace355_vae : LoadBase {   // (allocs: what the last finalize built)
    ace355_vae_config cfg;
    VaeShape shape;   // widths, strides and pads of both halves (vae_plan.h): what finalize builds and what the plans walk
    int hop = 1;
    std::map<std::string, RawT> raw;   // loaded and not yet consumed by a finalize
    // [0] decoder, [1] encoder (optional: present when encoder.* tensors were loaded); both indexed by vae_weight_slot
    std::vector<ConvW> conv[2];
    std::vector<SnakeP> snake[2];
    bool has_encoder = false;
    bf16_t* ain = nullptr;      // im2col'ed audio [B][L][64]
    size_t ain_elems = 0;
    float* e_head = nullptr;    // conv2 output f32 [B][2Z][T]
    size_t e_head_elems = 0;
    // activations
    bf16_t* buf[3] = {nullptr, nullptr, nullptr};
    size_t buf_elems = 0;
    // decode memory policy (ace355_vae_set_decode_budget): bytes the three ping-pong buffers may take before the decode is split
    // into windows (fewer items first, then overlap-discard windows in time)
    size_t decode_budget = (size_t)96 << 30;
    int decode_overlap = 0;          // latent frames of halo per window side; 0: max(16, receptive field + 2)
    int last_plan[3] = {0, 0, 0};    // (items per window, core frames, overlap) of the last decode
    bf16_t* zin = nullptr;
    size_t zin_elems = 0;
    // profile
    bool profile = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    double flops = 0;
    long launches = 0;
    // stage taps (ace355_vae_set_tap): [0] decoder, [1] encoder; stage -> (destination, capacity in bytes)
    std::map<int, std::pair<void*, size_t>> taps[2];
};

namespace {

// One row of the weight table (vae_plan.h) from its raw tensors `t` (vae_row_tensors order) into slot `slot` of its half; `nrm`: scratch
// for the row norms, shared by the rows (one stream)
int build_row(ace355_vae* h, int half, int slot, const VaeWeightRow& r, float* const* t, bool fused, float* nrm) {
    const VaePackDims& d = r.d;
    if (r.kind == VAE_ROW_SNAKE) {
        SnakeP& sp = h->snake[half][slot];
        ALLOC(h->allocs, sp.ea, (size_t)d.d0 * d.s);
        ALLOC(h->allocs, sp.ib, (size_t)d.d0 * d.s);
        return launch_snake_prep(t[0], t[1], sp.ea, sp.ib, d.d0, d.s, 0);
    }
    ConvW& c = h->conv[half][slot];
    const VaePacked pk = vae_packed(r);
    const float* g = fused ? nullptr : t[1];
    const long n = vae_norm_rows(r) * vae_norm_cols(r);
    ALLOC(h->allocs, c.w, (size_t)pk.elems);
    if (pk.elems != n) ACE_HIP(hipMemsetAsync(c.w, 0, (size_t)pk.elems * 2, 0));   // (IM2COL's pad columns)
    if (g) hipLaunchKernelGGL(rownorm_kernel, dim3((vae_norm_rows(r) + 3) / 4), dim3(256), 0, 0, t[0], vae_norm_cols(r), nrm, vae_norm_rows(r));
    hipLaunchKernelGGL(pack_weight_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, t[0], g, nrm, c.w, r.kind, d, n);
    if (r.bias_reps) {
        const int C = pk.N / r.bias_reps;
        ALLOC(h->allocs, c.bias, (size_t)pk.N);
        hipLaunchKernelGGL(tile_bias_kernel, dim3((pk.N + 255) / 256), dim3(256), 0, 0, t[fused ? 1 : 2], c.bias, C, r.bias_reps);
    }
    ACE_LAUNCH_CHECK();
    return 0;
}

int run_conv(ace355_vae* h, const ConvArgs& a, hipStream_t s) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (h->profile) {
        hipEventCreate(&e0); hipEventCreate(&e1);
        hipEventRecord(e0, s);
        h->flops += 2.0 * a.B * (double)a.M * (a.out_mode == 1 ? a.n_real : a.N) * a.taps * a.Cin;
        if (a.w2) h->flops += 2.0 * a.B * (double)a.M * a.N * a.N;  // fused k = 1 stage
        h->launches++;
    }
    int rc = launch_conv(a, s);
    if (h->profile) {
        hipEventRecord(e1, s);
        h->ev.push_back({e0, e1});
    }
    return rc;
}

}  // namespace

extern "C" {

int ace355_vae_create(const ace355_vae_config* cfg, ace355_vae** out) {
    ACE_CHECK(cfg && out, "vae_create: null argument");
    const char* bad = vae_config_error(*cfg);
    ACE_CHECK(!bad, bad);
    ace355_vae* h = new ace355_vae();
    h->cfg = *cfg;
    h->shape = vae_shape(*cfg);
    h->hop = h->shape.hop;
    if (const char* e = getenv("ACE355_VAE_BUDGET_MB")) { const long mb = atol(e); if (mb > 0) h->decode_budget = (size_t)mb << 20; }
    *out = h;
    return ACE355_OK;
}

void ace355_vae_destroy(ace355_vae* h) {
    if (!h) return;
    hipDeviceSynchronize();
    for (auto& kv : h->raw) hipFree(kv.second.p);
    free_base(h);
    for (int i = 0; i < 3; ++i) if (h->buf[i]) hipFree(h->buf[i]);
    if (h->zin) hipFree(h->zin);
    if (h->ain) hipFree(h->ain);
    if (h->e_head) hipFree(h->e_head);
    for (auto& e : h->ev) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    delete h;
}

int ace355_vae_load_tensor(ace355_vae* h, const char* name, const void* data, int dtype, int64_t numel, int is_device) {
    ACE_CHECK(h && name && data && numel > 0, "vae_load_tensor: null/empty argument");
    ACE_CHECK(dtype == ACE355_DTYPE_F32 || dtype == ACE355_DTYPE_BF16, "vae_load_tensor: dtype");
    const std::string key(name);
    if (key.rfind("decoder.", 0) != 0 && key.rfind("encoder.", 0) != 0) {
        set_error("vae_load_tensor: unknown tensor name '" + key + "' (decoder.* / encoder.* expected)");
        return ACE355_ERR_INVALID;
    }
    DevTmp tmp;   // [0]: the fp32 copy until the map owns it, [1]: bf16 staging
    float* p = nullptr;
    ALLOC(tmp.bag, p, (size_t)numel);
    const hipMemcpyKind kind = is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (dtype == ACE355_DTYPE_F32) {
        ACE_HIP(hipMemcpy(p, data, (size_t)numel * 4, kind));
    } else {
        bf16_t* st = nullptr;
        ALLOC(tmp.bag, st, (size_t)numel);
        ACE_HIP(hipMemcpy(st, data, (size_t)numel * 2, kind));
        hipLaunchKernelGGL(cvt_bf16_f32_kernel, dim3((unsigned)((numel + 255) / 256)), dim3(256), 0, 0, st, p, (long)numel);
        ACE_HIP(hipDeviceSynchronize());
    }
    RawT& r = h->raw[key];
    tmp.bag[0] = r.p;   // (a tensor loaded twice: the earlier copy goes)
    r.p = p;
    r.n = numel;
    h->finalized = false;
    return ACE355_OK;
}

// Host bookkeeping first: every tensor the weight table (vae_plan.h) names is there with its size, or nothing is touched.  Then what an
// earlier finalize built goes, the rows are built, and the raw tensors - consumed or unused - leave the map: a later finalize needs a
// full reload.
int ace355_vae_finalize(ace355_vae* h) {
    ACE_CHECK(h, "vae_finalize: null handle");
    const auto enc_key = h->raw.lower_bound("encoder.");
    const bool has_encoder = enc_key != h->raw.end() && enc_key->first.rfind("encoder.", 0) == 0;
    struct Src { float* t[3]; bool fused; };
    std::vector<VaeWeightRow> rows[2];
    std::vector<Src> src[2];
    int max_rows = 1;
    for (int half = 0; half < (has_encoder ? 2 : 1); ++half) {
        rows[half] = vae_weight_table(h->shape, half != 0);
        for (const VaeWeightRow& r : rows[half]) {
            ACE_CHECK(r.kind != VAE_ROW_IM2COL || r.d.d1 * r.d.K <= VAE_IM2COL_COLS, "vae_finalize: audio_channels * 7 must fit 64 virtual channels");
            Src s{{nullptr, nullptr, nullptr}, r.kind != VAE_ROW_SNAKE && h->raw.count(r.base + ".weight") != 0};
            int k = 0;
            for (const VaeRawTensor& t : vae_row_tensors(r, s.fused)) {
                const auto it = h->raw.find(t.name);
                if (it == h->raw.end()) { set_error("vae_finalize: missing tensor '" + t.name + "'"); return ACE355_ERR_STATE; }
                if (it->second.n != t.n) {
                    set_error("vae_finalize: wrong size for '" + t.name + "': got " + std::to_string(it->second.n) + ", expected " + std::to_string(t.n));
                    return ACE355_ERR_INVALID;
                }
                s.t[k++] = it->second.p;
            }
            src[half].push_back(s);
            max_rows = std::max(max_rows, vae_norm_rows(r));
        }
    }
    ACE_HIP(hipDeviceSynchronize());
    h->finalized = false;
    for (void* p : h->allocs) hipFree(p);
    h->allocs.clear();
    DevTmp tmp;
    float* nrm = nullptr;
    ALLOC(tmp.bag, nrm, (size_t)max_rows);
    for (int half = 0; half < 2; ++half) {
        h->conv[half].assign(rows[half].size(), ConvW());
        h->snake[half].assign(rows[half].size(), SnakeP());
        for (size_t i = 0; i < rows[half].size(); ++i) {
            const int rc = build_row(h, half, (int)i, rows[half][i], src[half][i].t, src[half][i].fused, nrm);
            if (rc) return rc;
        }
    }
    ACE_HIP(hipDeviceSynchronize());
    for (auto& kv : h->raw) hipFree(kv.second.p);
    h->raw.clear();
    h->has_encoder = has_encoder;
    h->finalized = true;
    return ACE355_OK;
}

int ace355_vae_hop(const ace355_vae* h) { return h ? h->hop : 0; }

// A stage that was just stored: copy it out when it is tapped.
static int tap_copy(ace355_vae* h, int enc, const ace355_vae_stage_info& si, int k, const void* p, int B, hipStream_t s) {
    auto it = h->taps[enc].find(k);
    if (it == h->taps[enc].end()) return 0;
    const size_t bytes = (size_t)B * si.rows * si.channels * ((si.flags & ACE355_VAE_FLAG_F32_NCL) ? 4 : 2);
    ACE_CHECK(bytes <= it->second.second, "vae tap: the destination is smaller than the stage");
    ACE_HIP(hipMemcpyAsync(it->second.first, p, bytes, hipMemcpyDeviceToDevice, s));
    return 0;
}
// Start of a decode / encode: with a tap on this half the call must be one whole-sequence window over the whole batch
static int tap_begin(ace355_vae* h, int enc, bool single_window) {
    if (h->taps[enc].empty() || single_window) return 0;
    set_error("vae tap: the call splits into several windows under the activation budget; a tap needs one whole-sequence window");
    return ACE355_ERR_STATE;
}

// The executor: one decode window / encode group, the steps of its plan in order (vae_plan.h).  `in` / `out`: the call's input image and
// output at the window's first item.  Roles become pointers, a step becomes ConvArgs, a tapped stage is copied out behind its launch.
static int run_plan(ace355_vae* h, int enc, const VaePlan& p, int B, const bf16_t* in, void* out, hipStream_t s) {
    const bool tapped = !h->taps[enc].empty();
    ACE_CHECK(!tapped || h->taps[enc].rbegin()->first < (int)p.stages.size(), "vae tap: no such stage");
    int rc;
    if (tapped && (rc = tap_copy(h, enc, p.stages[0], 0, in, B, s))) return rc;
    const VaeShape& sh = h->shape;
    // a role to its slot of the weight table (vae_plan.h)
    auto conv = [&](int role, int block, int unit) -> const ConvW& { return h->conv[enc][vae_weight_slot(sh, enc != 0, false, role, block, unit)]; };
    auto snake = [&](int role, int block, int unit) -> const SnakeP* {
        return role == ACE355_VAE_SNAKE_NONE ? nullptr : &h->snake[enc][vae_weight_slot(sh, enc != 0, true, role, block, unit)];
    };
    auto buf = [&](int role) -> bf16_t* {
        return role == ACE355_VAE_BUF_NONE ? nullptr : role == ACE355_VAE_BUF_IN ? const_cast<bf16_t*>(in) : role == ACE355_VAE_BUF_OUT ? (bf16_t*)out : h->buf[role];
    };
    for (const VaeStep& st : p.steps) {
        const ConvW& W = conv(st.weight, st.block, st.unit);
        ConvArgs a{};
        a.x = buf(st.src) + st.src_off; a.x_batch_stride = st.x_batch_stride; a.L_in = st.L_in; a.Cin = st.Cin;
        a.x_shift = st.x_shift; a.x_valid = st.x_valid;
        a.w = W.w; a.bias = W.bias;
        if (const SnakeP* sp = snake(st.in_snake, st.in_snake_block, st.unit)) a.alpha = sp->ea, a.beta = sp->ib;
        if (const SnakeP* sp = snake(st.out_snake, st.out_snake_block, st.unit)) a.osnake_a = sp->ea, a.osnake_b = sp->ib;
        if (st.fused) {   // the unit's second stage: snake2 and conv2
            const ConvW& W2 = conv(ACE355_VAE_W_UNIT_C2, st.block, st.unit);
            const SnakeP* s2 = snake(ACE355_VAE_SNAKE_UNIT_S2, st.block, st.unit);
            a.w2 = W2.w; a.bias2 = W2.bias; a.alpha2 = s2->ea; a.beta2 = s2->ib;
        }
        a.res = buf(st.res); a.res_batch_stride = st.res_batch_stride;
        a.y = buf(st.dst); a.y_batch_stride = st.y_batch_stride;
        a.B = B; a.M = st.M; a.N = st.N; a.taps = st.taps; a.dil = st.dil; a.center = st.center;
        a.y_shift = st.y_shift; a.y_valid = st.y_valid; a.out_mode = st.out_mode; a.n_real = st.n_real;
        a.ncl_ld = st.ncl_ld; a.ncl_off = st.ncl_off; a.ncl_m_lo = st.ncl_m_lo; a.ncl_m_hi = st.ncl_m_hi;
        if ((rc = run_conv(h, a, s))) return rc;
        if (tapped && st.stage >= 0 && (rc = tap_copy(h, enc, st.stage_info, st.stage, a.y, B, s))) return rc;
    }
    return 0;
}

int ace355_vae_decode(ace355_vae* h, const float* z_dev, int B, int T, float* wav_out_dev, void* stream) {
    RoctxRange r_dec("ace355.vae_decode");
    ACE_CHECK(h && z_dev && wav_out_dev, "vae_decode: null argument");
    if (!h->finalized) { set_error("vae_decode: call ace355_vae_finalize first"); return ACE355_ERR_STATE; }
    ACE_CHECK(B > 0 && T > 0, "vae_decode: empty problem");
    ACE_CHECK((long)T * h->hop < (1L << 31), "vae_decode: sequence too long (2^31 samples per item)");
    hipStream_t s = (hipStream_t)stream;
    const VaeShape& sh = h->shape;
    size_t budget = h->decode_budget;
    VaeWindowPlan wp;
    // allocation with the reference's out-of-memory policy (H/vae_decode_chunks.py:40-81 retries smaller instead of failing):
    // a refused hipMalloc halves the budget and re-plans, down to one minimal window
    for (int attempt = 0;; ++attempt) {
        wp = plan_vae_windows(sh, B, T, budget, h->decode_overlap);
        ACE_CHECK(!wp.error, wp.error);
        const long win = vae_window_frames(wp, T);
        const size_t need_elems = vae_decode_elems(sh, win) * (size_t)wp.nb;
        if (need_elems <= h->buf_elems) break;
        ACE_HIP(hipStreamSynchronize(s));
        bool ok = true;
        for (int i = 0; i < 3; ++i) {
            if (h->buf[i]) hipFree(h->buf[i]);
            h->buf[i] = nullptr;
        }
        h->buf_elems = 0;
        for (int i = 0; i < 3 && ok; ++i) ok = hipMalloc((void**)&h->buf[i], need_elems * 2 + 256) == hipSuccess;
        if (ok) { h->buf_elems = need_elems; break; }
        (void)hipGetLastError();
        for (int i = 0; i < 3; ++i) { if (h->buf[i]) hipFree(h->buf[i]); h->buf[i] = nullptr; }
        budget = std::min(budget, vae_decode_bytes(sh, wp.nb, win)) / 2;
        if (attempt >= 12 || budget < vae_decode_bytes(sh, 1, 3L * wp.ov + 8)) {
            set_error("vae_decode: out of device memory even for one minimal decode window");
            return ACE355_ERR_HIP;
        }
    }
    const size_t zel = (size_t)B * T * sh.zc;
    if (zel > h->zin_elems) {
        ACE_HIP(hipStreamSynchronize(s));
        if (h->zin) hipFree(h->zin);
        h->zin = nullptr; h->zin_elems = 0;
        ACE_HIP(hipMalloc((void**)&h->zin, zel * 2 + 256));
        h->zin_elems = zel;
    }
    int rc = tap_begin(h, 0, wp.nb == B && wp.tc == T);
    if (rc) return rc;
    if ((rc = launch_ncl_to_nlc(z_dev, h->zin, B, sh.zc, T, s))) return rc;
    h->last_plan[0] = wp.nb; h->last_plan[1] = wp.tc; h->last_plan[2] = wp.ov;
    for (int b0 = 0; b0 < B; b0 += wp.nb) {
        const int nbw = std::min(wp.nb, B - b0);
        for (int cs = 0; cs < T; cs += wp.tc) {
            const VaePlan p = plan_vae(sh, false, nbw, T, vae_window_at(wp, T, cs), conv_knobs());
            if ((rc = run_plan(h, 0, p, nbw, h->zin + (size_t)b0 * T * sh.zc, wav_out_dev + (size_t)b0 * sh.audio * sh.hop * T, s))) return rc;
        }
    }
    return ACE355_OK;
}

int ace355_vae_set_decode_budget(ace355_vae* h, int64_t bytes, int overlap_frames) {
    ACE_CHECK(h, "vae_set_decode_budget: null handle");
    ACE_CHECK(bytes >= 0 && overlap_frames >= 0, "vae_set_decode_budget: negative argument");
    if (bytes > 0) h->decode_budget = (size_t)bytes;
    if (overlap_frames > 0) {
        ACE_CHECK(overlap_frames >= vae_receptive_frames(h->shape) && overlap_frames % 8 == 0,
                  "vae_set_decode_budget: the overlap must cover the receptive field and be a multiple of 8 frames");
        h->decode_overlap = overlap_frames;
    }
    return ACE355_OK;
}

int ace355_vae_decode_plan(ace355_vae* h, int B, int T, int32_t* items_per_window, int32_t* core_frames, int32_t* overlap_frames,
                           int64_t* activation_bytes) {
    ACE_CHECK(h && B > 0 && T > 0, "vae_decode_plan: bad argument");
    if (!h->finalized) { set_error("vae_decode_plan: call ace355_vae_finalize first"); return ACE355_ERR_STATE; }
    const VaeWindowPlan wp = plan_vae_windows(h->shape, B, T, h->decode_budget, h->decode_overlap);
    ACE_CHECK(!wp.error, wp.error);
    if (items_per_window) *items_per_window = wp.nb;
    if (core_frames) *core_frames = wp.tc;
    if (overlap_frames) *overlap_frames = wp.ov;
    if (activation_bytes) *activation_bytes = (int64_t)vae_decode_bytes(h->shape, wp.nb, vae_window_frames(wp, T));
    return ACE355_OK;
}

// One group of items of an encode: im2col, the plan's steps, the Gaussian head
static int encode_group(ace355_vae* h, const float* audio_dev, const float* noise_dev, int B, int64_t L, const VaePlan& p, float* latents_out_dev,
                        hipStream_t s) {
    const VaeShape& sh = h->shape;
    const long T = p.out_len;
    const size_t need_elems = (size_t)B * p.slot_elems;
    if (need_elems > h->buf_elems) {
        ACE_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < 3; ++i) {
            if (h->buf[i]) hipFree(h->buf[i]);
            h->buf[i] = nullptr;
            ACE_HIP(hipMalloc((void**)&h->buf[i], need_elems * 2 + 256));
        }
        h->buf_elems = need_elems;
    }
    const size_t ael = (size_t)B * L * 64;
    if (ael > h->ain_elems) {
        ACE_HIP(hipStreamSynchronize(s));
        if (h->ain) hipFree(h->ain);
        ACE_HIP(hipMalloc((void**)&h->ain, ael * 2 + 256));
        h->ain_elems = ael;
    }
    const size_t hel = (size_t)B * sh.eh * T;
    if (hel > h->e_head_elems) {
        ACE_HIP(hipStreamSynchronize(s));
        if (h->e_head) hipFree(h->e_head);
        ACE_HIP(hipMalloc((void**)&h->e_head, hel * 4 + 256));
        h->e_head_elems = hel;
    }
    hipLaunchKernelGGL(audio_im2col_kernel, dim3((unsigned)((ael + 255) / 256)), dim3(256), 0, s, audio_dev, h->ain, sh.audio, (long)L, 7, (long)ael);
    ACE_LAUNCH_CHECK();
    int rc = run_plan(h, 1, p, B, h->ain, h->e_head, s);
    if (rc) return rc;
    const long total = (long)B * sh.zc * T;
    hipLaunchKernelGGL(gaussian_head_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, h->e_head, noise_dev, latents_out_dev, sh.zc, T, total);
    ACE_LAUNCH_CHECK();
    return ACE355_OK;
}

int ace355_vae_encode(ace355_vae* h, const float* audio_dev, const float* noise_dev, int B, int64_t L, float* latents_out_dev,
                      void* stream) {
    ACE_CHECK(h && audio_dev && latents_out_dev, "vae_encode: null argument");
    if (!h->finalized) { set_error("vae_encode: call ace355_vae_finalize first"); return ACE355_ERR_STATE; }
    if (!h->has_encoder) { set_error("vae_encode: no encoder.* tensors were loaded"); return ACE355_ERR_STATE; }
    ACE_CHECK(B > 0 && L > 0 && L < (1L << 30), "vae_encode: sizes");
    // same activation budget as the decode (ace355_vae_set_decode_budget): above it the batch is encoded in groups of items (exact:
    // items are independent; the reference's 30 s / 2 s-overlap encode tiling, H/vae_encode.py:47-86, is the same kind of memory bound)
    const VaeShape& sh = h->shape;
    const long T = vae_latent_frames(sh, L);
    ACE_CHECK(T > 0, "vae_encode: audio shorter than one latent frame");
    const long slot_elems = plan_vae(sh, true, 1, L, VaeWindow{}, conv_knobs()).slot_elems;
    const int nb = vae_encode_group(B, L, slot_elems, h->decode_budget);
    int rc = tap_begin(h, 1, nb == B);
    if (rc) return rc;
    for (int b0 = 0; b0 < B; b0 += nb) {
        const int n = std::min(nb, B - b0);
        rc = encode_group(h, audio_dev + (size_t)b0 * sh.audio * L, noise_dev ? noise_dev + (size_t)b0 * sh.zc * T : nullptr, n, L,
                          plan_vae(sh, true, n, L, VaeWindow{}, conv_knobs()), latents_out_dev + (size_t)b0 * sh.zc * T, (hipStream_t)stream);
        if (rc) return rc;
    }
    return ACE355_OK;
}

int ace355_vae_latent_frames(const ace355_vae* h, int64_t L) {
    if (!h || !h->finalized || !h->has_encoder || L <= 0) return -1;
    return (int)vae_latent_frames(h->shape, L);
}

// The public stages are the plan's: of one whole-sequence window
static VaePlan stage_plan(const ace355_vae* h, int enc, long T) {
    return plan_vae(h->shape, enc != 0, 1, T, VaeWindow{0, (int)T, 0, (int)T}, conv_knobs());
}

int ace355_vae_num_stages(const ace355_vae* h, int encoder) {
    if (!h || !h->finalized || (encoder && !h->has_encoder)) return -1;
    const VaePlan p = stage_plan(h, encoder, encoder ? (long)h->hop * 4 : 4);   // (the count does not depend on the length)
    return p.error ? -1 : (int)p.stages.size();
}

int ace355_vae_get_stage(const ace355_vae* h, int encoder, int stage, int64_t T, ace355_vae_stage_info* out) {
    ACE_CHECK(h && out && T > 0, "vae_get_stage: bad argument");
    if (!h->finalized || (encoder && !h->has_encoder)) { set_error("vae_get_stage: not finalized, or no encoder.* tensors were loaded"); return ACE355_ERR_STATE; }
    const VaePlan p = stage_plan(h, encoder, (long)T);
    ACE_CHECK(!p.error, "vae stages: audio shorter than one latent frame");
    ACE_CHECK(stage >= 0 && stage < (int)p.stages.size(), "vae_get_stage: no such stage");
    *out = p.stages[stage];
    return ACE355_OK;
}

int ace355_vae_set_tap(ace355_vae* h, int encoder, int stage, void* dst_dev, int64_t capacity_bytes) {
    ACE_CHECK(h, "vae_set_tap: null handle");
    if (!h->finalized || (encoder && !h->has_encoder)) { set_error("vae_set_tap: not finalized, or no encoder.* tensors were loaded"); return ACE355_ERR_STATE; }
    ACE_CHECK(stage >= 0 && stage < ace355_vae_num_stages(h, encoder), "vae_set_tap: no such stage");
    ACE_CHECK(!dst_dev || capacity_bytes > 0, "vae_set_tap: capacity");
    if (dst_dev) h->taps[encoder ? 1 : 0][stage] = {dst_dev, (size_t)capacity_bytes};
    else h->taps[encoder ? 1 : 0].erase(stage);
    return ACE355_OK;
}

int ace355_vae_set_profile(ace355_vae* h, int enable) {
    ACE_CHECK(h, "vae_set_profile: null handle");
    hipDeviceSynchronize();
    for (auto& e : h->ev) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    h->ev.clear();
    h->flops = 0;
    h->launches = 0;
    h->profile = enable != 0;
    return ACE355_OK;
}

int ace355_vae_get_profile(ace355_vae* h, double* conv_ms, double* conv_flops, int64_t* conv_launches) {
    ACE_CHECK(h, "vae_get_profile: null handle");
    ACE_HIP(hipDeviceSynchronize());
    double g = 0;
    float ms;
    for (auto& e : h->ev) if (hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) g += ms;
    if (conv_ms) *conv_ms = g;
    if (conv_flops) *conv_flops = h->flops;
    if (conv_launches) *conv_launches = h->launches;
    return ACE355_OK;
}

}  // extern "C"
