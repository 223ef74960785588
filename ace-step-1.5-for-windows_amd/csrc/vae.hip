// vae.hip - the Oobleck VAE handle behind ace355.h: weight-norm fusion + packing at load time, whole-sequence decode
// (architecture per acestep/models/mlx/vae_model.py:190-230) and - SURVEY.md section 8f row N3 - whole-sequence encode
// (vae_model.py:92-116, 148-187, 285-310) as chains of conv_kernel launches (conv.hip).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "encoder.h"   // dev_alloc
#include "vae_plan.h"

using namespace ace355;

namespace {

struct ConvW {
    bf16_t* w = nullptr;   // [N][taps][Cin]
    float* bias = nullptr; // [N] or null
    int N = 0, taps = 0, Cin = 0;
};
struct SnakeP {
    float* ea = nullptr;  // exp(alpha)
    float* ib = nullptr;  // 1 / (exp(beta) + 1e-9)
};
struct ResUnitW {
    SnakeP s1, s2;
    ConvW c1, c2;
};
struct BlockW {
    SnakeP s1;
    ConvW ct;
    ResUnitW ru[3];
};
struct EncBlockW {
    ResUnitW ru[3];
    SnakeP s1;       // tiled `stride` times (virtual channel c' -> channel c' % cin)
    ConvW cd;        // strided conv as 2 taps over stride*cin virtual channels
};
struct RawT {
    float* p = nullptr;
    long n = 0;
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
// Conv1d weight_v [Cout][Cin][K] (+g, norm) -> w[co][k][ci] bf16
__global__ void pack_conv_kernel(const float* __restrict__ v, const float* __restrict__ g, const float* __restrict__ nrm,
                                 bf16_t* __restrict__ w, int Cout, int Cin, int K) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)Cout * Cin * K) return;
    const int k = (int)(i % K);
    const long t = i / K;
    const int ci = (int)(t % Cin), co = (int)(t / Cin);
    float x = v[i];
    if (g) x = g[co] * x / (nrm[co] + 1e-9f);
    w[((long)co * K + k) * Cin + ci] = f2bf(x);
}
// ConvTranspose1d weight_v [Cin][Cout][2s] (+g over dim 0) -> w[r*Cout + co][tap][ci]; tap0 <-> k = r + s (x[i0-1]), tap1 <-> k = r (x[i0])
__global__ void pack_convt_kernel(const float* __restrict__ v, const float* __restrict__ g, const float* __restrict__ nrm,
                                  bf16_t* __restrict__ w, int Cin, int Cout, int s) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int K = 2 * s;
    if (i >= (long)Cin * Cout * K) return;
    const int k = (int)(i % K);
    const long t = i / K;
    const int co = (int)(t % Cout), ci = (int)(t / Cout);
    float x = v[i];
    if (g) x = g[ci] * x / (nrm[ci] + 1e-9f);
    const int r = k % s, tap = k >= s ? 0 : 1;
    w[(((long)r * Cout + co) * 2 + tap) * Cin + ci] = f2bf(x);
}
// strided Conv1d weight_v [Cout][C][2s] (+g, norm) -> w[co][g][s' * C + ci] with k = g*s + s'  (2 taps over s*C virtual channels)
__global__ void pack_conv_strided_kernel(const float* __restrict__ v, const float* __restrict__ g, const float* __restrict__ nrm,
                                         bf16_t* __restrict__ w, int Cout, int C, int s) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int K = 2 * s;
    if (i >= (long)Cout * C * K) return;
    const int k = (int)(i % K);
    const long t = i / K;
    const int ci = (int)(t % C), co = (int)(t / C);
    float x = v[i];
    if (g) x = g[co] * x / (nrm[co] + 1e-9f);
    const int gg = k / s, sp = k % s;
    w[((long)co * 2 + gg) * ((long)s * C) + (long)sp * C + ci] = f2bf(x);
}
// first encoder conv (Cin = audio channels, k = 7) as a 1-tap conv over 64 virtual channels: w'[co][k*A + c] = w[co][c][k]
__global__ void pack_conv_im2col_kernel(const float* __restrict__ v, const float* __restrict__ g, const float* __restrict__ nrm,
                                        bf16_t* __restrict__ w, int Cout, int A, int K) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)Cout * 64) return;
    const int cc = (int)(i % 64), co = (int)(i / 64);
    float x = 0.f;
    if (cc < K * A) {
        const int k = cc / A, c = cc % A;
        x = v[((long)co * A + c) * K + k];
        if (g) x = g[co] * x / (nrm[co] + 1e-9f);
    }
    w[i] = f2bf(x);
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
__global__ void snake_prep_kernel(const float* __restrict__ alpha, const float* __restrict__ beta, float* __restrict__ ea,
                                  float* __restrict__ ib, int C) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C) return;
    ea[i] = expf(alpha[i]);
    ib[i] = 1.0f / (expf(beta[i]) + 1e-9f);
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

struct ace355_vae {
    ace355_vae_config cfg;
    VaeShape shape;   // widths, strides and pads of both halves (vae_plan.h): what finalize builds and what the plans walk
    int hop = 1;
    std::map<std::string, RawT> raw;
    std::vector<void*> allocs;
    ConvW conv1, conv2;
    SnakeP s_out;
    std::vector<BlockW> blocks;
    bool finalized = false;
    // encoder (optional: present when encoder.* tensors were loaded)
    bool has_encoder = false;
    ConvW e_conv1, e_conv2;
    SnakeP e_s_out;
    std::vector<EncBlockW> e_blocks;
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
    float* scratch = nullptr;
    // profile
    bool profile = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    double flops = 0;
    long launches = 0;
    // stage taps (ace355_vae_set_tap): [0] decoder, [1] encoder; stage -> (destination, capacity in bytes)
    std::map<int, std::pair<void*, size_t>> taps[2];
};

namespace {

template <typename T>
int valloc(ace355_vae* h, T** p, size_t n) {
    return dev_alloc(h->allocs, p, n);
}

const RawT* find(ace355_vae* h, const std::string& k) {
    auto it = h->raw.find(k);
    return it == h->raw.end() ? nullptr : &it->second;
}

int need(ace355_vae* h, const std::string& k, long n, const RawT** out) {
    const RawT* r = find(h, k);
    if (!r) { set_error("vae_finalize: missing tensor '" + k + "'"); return ACE355_ERR_STATE; }
    if (r->n != n) { set_error("vae_finalize: wrong size for '" + k + "': got " + std::to_string(r->n) + ", expected " + std::to_string(n)); return ACE355_ERR_INVALID; }
    *out = r;
    return 0;
}

// Conv1d: base.weight_g [Cout,1,1], base.weight_v [Cout,Cin,K] (or fused base.weight), base.bias [Cout]
int build_conv(ace355_vae* h, const std::string& base, int Cout, int Cin, int K, bool has_bias, ConvW* c) {
    const RawT *v = nullptr, *g = nullptr, *b = nullptr;
    int rc;
    const bool fused = find(h, base + ".weight") != nullptr;
    if (fused) {
        if ((rc = need(h, base + ".weight", (long)Cout * Cin * K, &v))) return rc;
    } else {
        if ((rc = need(h, base + ".weight_v", (long)Cout * Cin * K, &v))) return rc;
        if ((rc = need(h, base + ".weight_g", Cout, &g))) return rc;
    }
    if (has_bias && (rc = need(h, base + ".bias", Cout, &b))) return rc;
    c->N = Cout; c->taps = K; c->Cin = Cin;
    if ((rc = valloc(h, &c->w, (size_t)Cout * Cin * K))) return rc;
    float* nrm = nullptr;
    if (g) {
        if ((rc = valloc(h, &nrm, (size_t)Cout))) return rc;
        hipLaunchKernelGGL(rownorm_kernel, dim3((Cout + 3) / 4), dim3(256), 0, 0, v->p, (long)Cin * K, nrm, Cout);
    }
    const long n = (long)Cout * Cin * K;
    hipLaunchKernelGGL(pack_conv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, v->p, g ? g->p : nullptr, nrm, c->w, Cout, Cin, K);
    c->bias = has_bias ? b->p : nullptr;
    ACE_LAUNCH_CHECK();
    return 0;
}

int build_convt(ace355_vae* h, const std::string& base, int Cin, int Cout, int s, ConvW* c) {
    const RawT *v = nullptr, *g = nullptr, *b = nullptr;
    int rc;
    const int K = 2 * s;
    const bool fused = find(h, base + ".weight") != nullptr;
    if (fused) {
        if ((rc = need(h, base + ".weight", (long)Cin * Cout * K, &v))) return rc;
    } else {
        if ((rc = need(h, base + ".weight_v", (long)Cin * Cout * K, &v))) return rc;
        if ((rc = need(h, base + ".weight_g", Cin, &g))) return rc;
    }
    if ((rc = need(h, base + ".bias", Cout, &b))) return rc;
    c->N = s * Cout; c->taps = 2; c->Cin = Cin;
    if ((rc = valloc(h, &c->w, (size_t)Cin * Cout * K))) return rc;
    float* nrm = nullptr;
    if (g) {
        if ((rc = valloc(h, &nrm, (size_t)Cin))) return rc;
        hipLaunchKernelGGL(rownorm_kernel, dim3((Cin + 3) / 4), dim3(256), 0, 0, v->p, (long)Cout * K, nrm, Cin);
    }
    const long n = (long)Cin * Cout * K;
    hipLaunchKernelGGL(pack_convt_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, v->p, g ? g->p : nullptr, nrm, c->w, Cin, Cout, s);
    if ((rc = valloc(h, &c->bias, (size_t)s * Cout))) return rc;
    hipLaunchKernelGGL(tile_bias_kernel, dim3((s * Cout + 255) / 256), dim3(256), 0, 0, b->p, c->bias, Cout, s);
    ACE_LAUNCH_CHECK();
    return 0;
}

int build_snake(ace355_vae* h, const std::string& base, int C, SnakeP* sp) {
    const RawT *a = nullptr, *b = nullptr;
    int rc;
    if ((rc = need(h, base + ".alpha", C, &a))) return rc;
    if ((rc = need(h, base + ".beta", C, &b))) return rc;
    if ((rc = valloc(h, &sp->ea, (size_t)C))) return rc;
    if ((rc = valloc(h, &sp->ib, (size_t)C))) return rc;
    hipLaunchKernelGGL(snake_prep_kernel, dim3((C + 255) / 256), dim3(256), 0, 0, a->p, b->p, sp->ea, sp->ib, C);
    ACE_LAUNCH_CHECK();
    return 0;
}

int build_conv_strided(ace355_vae* h, const std::string& base, int Cout, int C, int s, ConvW* c) {
    const RawT *v = nullptr, *g = nullptr, *b = nullptr;
    int rc;
    const int K = 2 * s;
    const bool fused = find(h, base + ".weight") != nullptr;
    if (fused) {
        if ((rc = need(h, base + ".weight", (long)Cout * C * K, &v))) return rc;
    } else {
        if ((rc = need(h, base + ".weight_v", (long)Cout * C * K, &v))) return rc;
        if ((rc = need(h, base + ".weight_g", Cout, &g))) return rc;
    }
    if ((rc = need(h, base + ".bias", Cout, &b))) return rc;
    c->N = Cout; c->taps = 2; c->Cin = s * C;
    if ((rc = valloc(h, &c->w, (size_t)Cout * C * K))) return rc;
    float* nrm = nullptr;
    if (g) {
        if ((rc = valloc(h, &nrm, (size_t)Cout))) return rc;
        hipLaunchKernelGGL(rownorm_kernel, dim3((Cout + 3) / 4), dim3(256), 0, 0, v->p, (long)C * K, nrm, Cout);
    }
    const long n = (long)Cout * C * K;
    hipLaunchKernelGGL(pack_conv_strided_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, v->p, g ? g->p : nullptr, nrm, c->w, Cout, C, s);
    c->bias = b->p;
    ACE_LAUNCH_CHECK();
    return 0;
}

int build_conv_im2col(ace355_vae* h, const std::string& base, int Cout, int A, int K, ConvW* c) {
    const RawT *v = nullptr, *g = nullptr, *b = nullptr;
    int rc;
    ACE_CHECK(A * K <= 64, "vae_finalize: audio_channels * 7 must fit 64 virtual channels");
    const bool fused = find(h, base + ".weight") != nullptr;
    if (fused) {
        if ((rc = need(h, base + ".weight", (long)Cout * A * K, &v))) return rc;
    } else {
        if ((rc = need(h, base + ".weight_v", (long)Cout * A * K, &v))) return rc;
        if ((rc = need(h, base + ".weight_g", Cout, &g))) return rc;
    }
    if ((rc = need(h, base + ".bias", Cout, &b))) return rc;
    c->N = Cout; c->taps = 1; c->Cin = 64;
    if ((rc = valloc(h, &c->w, (size_t)Cout * 64))) return rc;
    float* nrm = nullptr;
    if (g) {
        if ((rc = valloc(h, &nrm, (size_t)Cout))) return rc;
        hipLaunchKernelGGL(rownorm_kernel, dim3((Cout + 3) / 4), dim3(256), 0, 0, v->p, (long)A * K, nrm, Cout);
    }
    const long n = (long)Cout * 64;
    hipLaunchKernelGGL(pack_conv_im2col_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, v->p, g ? g->p : nullptr, nrm, c->w, Cout, A, K);
    c->bias = b->p;
    ACE_LAUNCH_CHECK();
    return 0;
}

// Snake parameters repeated `reps` times (the strided conv's virtual channels)
int build_snake_tiled(ace355_vae* h, const std::string& base, int C, int reps, SnakeP* sp) {
    SnakeP one;
    int rc = build_snake(h, base, C, &one);
    if (rc) return rc;
    if ((rc = valloc(h, &sp->ea, (size_t)C * reps))) return rc;
    if ((rc = valloc(h, &sp->ib, (size_t)C * reps))) return rc;
    hipLaunchKernelGGL(tile_bias_kernel, dim3((C * reps + 255) / 256), dim3(256), 0, 0, one.ea, sp->ea, C, reps);
    hipLaunchKernelGGL(tile_bias_kernel, dim3((C * reps + 255) / 256), dim3(256), 0, 0, one.ib, sp->ib, C, reps);
    ACE_LAUNCH_CHECK();
    return 0;
}

int build_res_unit(ace355_vae* h, const std::string& r, int C, ResUnitW* R) {
    int rc;
    if ((rc = build_snake(h, r + ".snake1", C, &R->s1))) return rc;
    if ((rc = build_conv(h, r + ".conv1", C, C, 7, true, &R->c1))) return rc;
    if ((rc = build_snake(h, r + ".snake2", C, &R->s2))) return rc;
    return build_conv(h, r + ".conv2", C, C, 1, true, &R->c2);
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
    for (auto& kv : h->raw) if (kv.second.p) hipFree(kv.second.p);
    for (void* p : h->allocs) hipFree(p);
    for (int i = 0; i < 3; ++i) if (h->buf[i]) hipFree(h->buf[i]);
    if (h->zin) hipFree(h->zin);
    if (h->ain) hipFree(h->ain);
    if (h->e_head) hipFree(h->e_head);
    if (h->scratch) hipFree(h->scratch);
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
    RawT& r = h->raw[key];
    if (r.p) { hipFree(r.p); r.p = nullptr; }
    ACE_HIP(hipMalloc((void**)&r.p, (size_t)numel * 4 + 256));
    r.n = numel;
    if (dtype == ACE355_DTYPE_F32) {
        ACE_HIP(hipMemcpy(r.p, data, (size_t)numel * 4, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    } else {
        bf16_t* tmp = nullptr;
        ACE_HIP(hipMalloc((void**)&tmp, (size_t)numel * 2 + 256));
        ACE_HIP(hipMemcpy(tmp, data, (size_t)numel * 2, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        hipLaunchKernelGGL(cvt_bf16_f32_kernel, dim3((unsigned)((numel + 255) / 256)), dim3(256), 0, 0, tmp, r.p, (long)numel);
        ACE_HIP(hipDeviceSynchronize());
        hipFree(tmp);
    }
    h->finalized = false;
    return ACE355_OK;
}

int ace355_vae_finalize(ace355_vae* h) {
    ACE_CHECK(h, "vae_finalize: null handle");
    const VaeShape& sh = h->shape;
    const int nb = sh.nb;
    int rc;
    if ((rc = build_conv(h, "decoder.conv1", sh.dec_c0, sh.zc, 7, true, &h->conv1))) return rc;
    h->blocks.assign(nb, BlockW());
    for (int i = 0; i < nb; ++i) {
        BlockW& B = h->blocks[i];
        const VaeBlockShape& S = sh.dec[i];
        const std::string p = "decoder.block." + std::to_string(i);
        if ((rc = build_snake(h, p + ".snake1", S.cin, &B.s1))) return rc;
        if ((rc = build_convt(h, p + ".conv_t1", S.cin, S.cout, S.stride, &B.ct))) return rc;
        for (int j = 0; j < 3; ++j)
            if ((rc = build_res_unit(h, p + ".res_unit" + std::to_string(j + 1), S.cout, &B.ru[j]))) return rc;
    }
    if ((rc = build_snake(h, "decoder.snake1", sh.dec_cl, &h->s_out))) return rc;
    if ((rc = build_conv(h, "decoder.conv2", sh.audio, sh.dec_cl, 7, false, &h->conv2))) return rc;
    // encoder half (optional): vae_model.py:148-187.  encoder_hidden_size = 2 * latent channels (mean | scale)
    h->has_encoder = false;
    for (auto& kv : h->raw) if (kv.first.rfind("encoder.", 0) == 0) { h->has_encoder = true; break; }
    if (h->has_encoder) {
        if ((rc = build_conv_im2col(h, "encoder.conv1", sh.eh, sh.audio, 7, &h->e_conv1))) return rc;
        h->e_blocks.assign(nb, EncBlockW());
        for (int i = 0; i < nb; ++i) {
            EncBlockW& B = h->e_blocks[i];
            const VaeBlockShape& S = sh.enc[i];
            const std::string p = "encoder.block." + std::to_string(i);
            for (int j = 0; j < 3; ++j)
                if ((rc = build_res_unit(h, p + ".res_unit" + std::to_string(j + 1), S.cin, &B.ru[j]))) return rc;
            if ((rc = build_snake_tiled(h, p + ".snake1", S.cin, S.stride, &B.s1))) return rc;
            if ((rc = build_conv_strided(h, p + ".conv1", S.cout, S.cin, S.stride, &B.cd))) return rc;
        }
        if ((rc = build_snake(h, "encoder.snake1", sh.enc_cl, &h->e_s_out))) return rc;
        if ((rc = build_conv(h, "encoder.conv2", sh.eh, sh.enc_cl, 3, true, &h->e_conv2))) return rc;
    }
    ACE_HIP(hipDeviceSynchronize());
    // raw weight_v / weight_g copies are no longer needed (biases are still referenced)
    for (auto& kv : h->raw) {
        const std::string& k = kv.first;
        const bool keep = k.size() > 5 && k.compare(k.size() - 5, 5, ".bias") == 0;
        if (!keep && kv.second.p) { hipFree(kv.second.p); kv.second.p = nullptr; }
    }
    if (!h->scratch) ACE_HIP(hipMalloc((void**)&h->scratch, 1024));
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
    auto unit = [&](int block, int j) -> const ResUnitW& { return enc ? h->e_blocks[block].ru[j] : h->blocks[block].ru[j]; };
    auto buf = [&](int role) -> bf16_t* {
        return role == ACE355_VAE_BUF_NONE ? nullptr : role == ACE355_VAE_BUF_IN ? const_cast<bf16_t*>(in) : role == ACE355_VAE_BUF_OUT ? (bf16_t*)out : h->buf[role];
    };
    for (const VaeStep& st : p.steps) {
        auto snake = [&](int which, int block) -> const SnakeP* {
            switch (which) {
                case ACE355_VAE_SNAKE_UNIT_S1: return &unit(block, st.unit).s1;
                case ACE355_VAE_SNAKE_UNIT_S2: return &unit(block, st.unit).s2;
                case ACE355_VAE_SNAKE_BLOCK: return enc ? &h->e_blocks[block].s1 : &h->blocks[block].s1;   // (encoder: tiled `stride` times)
                case ACE355_VAE_SNAKE_FINAL: return enc ? &h->e_s_out : &h->s_out;
                default: return nullptr;
            }
        };
        const ConvW* W = nullptr;
        switch (st.weight) {
            case ACE355_VAE_W_CONV_IN: W = enc ? &h->e_conv1 : &h->conv1; break;
            case ACE355_VAE_W_CONVT: W = &h->blocks[st.block].ct; break;
            case ACE355_VAE_W_UNIT_C1: W = &unit(st.block, st.unit).c1; break;
            case ACE355_VAE_W_UNIT_C2: W = &unit(st.block, st.unit).c2; break;
            case ACE355_VAE_W_DOWN: W = &h->e_blocks[st.block].cd; break;
            case ACE355_VAE_W_OUT: W = &h->conv2; break;
            default: W = &h->e_conv2; break;
        }
        ConvArgs a{};
        a.x = buf(st.src) + st.src_off; a.x_batch_stride = st.x_batch_stride; a.L_in = st.L_in; a.Cin = st.Cin;
        a.x_shift = st.x_shift; a.x_valid = st.x_valid;
        a.w = W->w; a.bias = W->bias;
        if (const SnakeP* sp = snake(st.in_snake, st.in_snake_block)) a.alpha = sp->ea, a.beta = sp->ib;
        if (const SnakeP* sp = snake(st.out_snake, st.out_snake_block)) a.osnake_a = sp->ea, a.osnake_b = sp->ib;
        if (st.fused) {
            const ResUnitW& R = unit(st.block, st.unit);
            a.w2 = R.c2.w; a.bias2 = R.c2.bias; a.alpha2 = R.s2.ea; a.beta2 = R.s2.ib;
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
