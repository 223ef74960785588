/*
 * ace355.h - C ABI of the MI355X-native (gfx950) ACE-Step 1.5 denoise + decode path.
 *
 * The reference (sdbds/ACE-Step-1.5-for-windows) has no FFI; its backend seam is a pair
 * of Python mixin methods added for MLX.  This header is what a ctypes binding
 * behind that seam talks to (INTEGRATION.md shows the stub).  Every entry point cites the
 * reference interface it replaces (paths relative to /root/reference/acestep/):
 *
 *   base.py = models/base/modeling_acestep_v15_base.py      H/ = core/generation/handler/
 *
 * Conventions
 *   - plain C: opaque handles, raw pointers, sizes; no torch / C++ types.
 *   - "dev" pointers are HIP device pointers on the current device; "host" pointers are
 *     ordinary host memory.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - every function returns ACE355_OK (0) or an error code; ace355_last_error() returns a
 *     thread-local message (HIP error string included).  Nothing aborts the process
 *     (reference contract: backend failure = exception caught at the seam,
 *     H/service_generate_execute.py:189-191, H/vae_decode.py:44-48).
 *   - handles are not thread-safe; one generation in flight per handle (SURVEY.md section 5,
 *     "Race detection": the reference serialises requests per handler).
 */
#ifndef ACE355_H
#define ACE355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACE355_OK 0
#define ACE355_ERR_INVALID 1 /* bad argument / shape / unknown tensor name */
#define ACE355_ERR_HIP 2     /* a HIP runtime call failed */
#define ACE355_ERR_STATE 3   /* call order violated (e.g. forward before finalize) */
#define ACE355_ERR_UNSUPPORTED 4

#define ACE355_DTYPE_F32 0
#define ACE355_DTYPE_BF16 1

#define ACE355_MAX_BLOCKS 8
#define ACE355_MAX_SEQS 64
#define ACE355_MAX_SLOTS 32 /* resident condition slots per DiT handle: 8 cover + 8 non-cover per-item conditions + null + spare */

const char* ace355_last_error(void);
int ace355_version(void);
/* Measurement aid (bench.py `box_probe`; no reference counterpart): dense bf16 MFMA rate of THIS board on a pure
 * v_mfma_f32_32x32x16_bf16 loop with random operands, 8 waves per CU, no memory traffic (TFLOP/s; the boxes of the pool differ by a
 * few percent under the same power cap, and a bench line is only comparable across boxes beside this number).  Synchronises the device. */
int ace355_box_probe_mfma(int iters, double* tflops_out);
/* Tuning knob of the bf16 GEMM (no reference counterpart; process-wide, returns the previous mode).  K rotation: in a launch that gives
 * every CU exactly one output tile (the o_proj / down projections at the metric batch), all eight L2s would miss the same K slice of the
 * operands at the same moment; with the rotation on, the workgroups of XCD x start at K step x * nk / 8 and wrap, so a slice's first reader
 * pays the HBM latency and the others find it in the memory-side cache (K step 1.12 -> 1.06 us, - 1 % per 8-song pass).  The fp32 accumulation
 * ORDER of an output element then depends on the XCD region its tile falls in, i.e. on the launch shape: the same request still gives the
 * same bits, but a song's bits depend on the batch it is part of (3e-3 rel L2 apart, both at the same distance from the reference).
 * mode 0: off (one K order whatever the shape; what the bit-identity tests of the CFG fork pin), 1 (default; env ACE355_GEMM_KROT):
 * launches with N <= 2048, 2: every one-round launch.  Not a per-handle setting: call it before the first request.
 * Mode 0 is the library's "launch-shape-independent arithmetic" switch as a whole: the attention launcher then also keeps to its one-walk
 * kernels (the 12-wave key-split kernel of the 96-row launches merges two partial softmaxes per row, and which launches are 96-row ones
 * depends on how many sequences share them), so a song computed alone and inside a larger batch agree bit for bit wherever both runs take
 * the GQA kernels (tests/test_metric_shapes_gpu.py::test_120s_forward_vs_reference_golden_and_batch16). */
int ace355_gemm_set_k_rotation(int mode);
/* Which launch the bf16 / MXFP8 GEMM entry points would make for a request (no reference counterpart; a test and review aid): the
 * library's launch decision is one pure function of the request and the process's ACE355_GEMM_* switches, and this call evaluates it.
 * No GPU is touched.  Fields are the library's GemmRequest / GemmPlan (csrc/gemm_plan.h), where each is described. */
#define ACE355_GEMM_PLACEMENT_PROCESS (-2) /* placement: what this process found (unknown until a handle or a residual GEMM asked) */
typedef struct ace355_gemm_request {
    int32_t M, N, K;
    int32_t mode;           /* 0 store bf16, 1 store f32, 2 residual into f32, 3 SwiGLU, 4 QKV with head-norm + RoPE */
    int32_t fp8;            /* 1: MXFP8 operands (modes 0 / 2 / 3 / 4, K % 128 == 0, N % 256 == 0) */
    int32_t cu_slots;       /* 8 .. 256: plan for that many CUs; 0: ACE355_MAX_WGS */
    int32_t aligned;        /* output and per-column vectors are 16-byte aligned */
    int32_t counters;       /* split-K turn counters are lent (the handles and the residual entry points do) */
    int32_t fold_producer, fold_consumer;
    int32_t hn_q_cols, hn_qk_cols;
    int32_t vt_offered, vt_heads;
    int32_t pf_x;           /* prefetch workgroups per XCD attached for the next launch's weights, 0: none */
    int32_t placement;      /* -1 unknown, 0 refused, 1 verified, or ACE355_GEMM_PLACEMENT_PROCESS */
} ace355_gemm_request;
typedef struct ace355_gemm_plan_info {
    int32_t mode, mt, wnw, ntw, pers, ns, fp8;                      /* gemm_sp_kernel<mode, mt, wnw, ntw, pers, ns, fp8> */
    int32_t grid_x, grid_y, threads, tiles_n, nwg, group_m, xcd_m;  /* launch geometry and tile map */
    int32_t ksplit, kparts, sk_ord, krot, wide_ok, pf_x;            /* epilogue fields the launcher sets */
    int32_t head_fused, vt_epilogue;
    /* the XCD column regions a PRECEDING launch would be given to prefetch this request's weights (all 0: none attached) */
    int32_t next_pf_x, next_pf_xcd_n;
    uint32_t next_pf_chunk16, next_pf_len16;
} ace355_gemm_plan_info;
int ace355_gemm_plan(const ace355_gemm_request* request, ace355_gemm_plan_info* plan_out);
/* The same for the attention entry points and the attention launches of the handles: the launch decision is one pure function of the
 * request, the process's ACE355_ATTN_* switches and whether K rotation mode 0 is set at the time of the call.  No GPU is touched.  Fields
 * are the library's AttnRequest / AttnPlan (csrc/attn_plan.h), where each is described. */
#define ACE355_ATTN_KERNEL_ATTN3 0 /* attn3_kernel<nw = 4 | 8>: one q head per workgroup, 32 nw query rows; the only one that splits KV */
#define ACE355_ATTN_KERNEL_GQA 1   /* attn_gqa_kernel<nw = 3 | 4 | 6>: both q heads of a KV head per workgroup, 32 nw query rows */
#define ACE355_ATTN_KERNEL_ROT 2   /* attn_rot_kernel<nw = 3>: 96 query rows, the key range split between two wave groups */
typedef struct ace355_attn_request {
    int32_t N, Sq, Skv, Hq, Hkv;
    int32_t window;         /* sliding band |i - j| <= window, -1: full attention */
    int32_t cu_slots;       /* 8 .. 256: plan for that many CUs; 0: ACE355_MAX_WGS */
    int32_t has_kv_len;     /* a key-padding mask is set (ace355_attention_masked, the condition encoders) */
    int32_t mx_out;         /* MXFP8 output is asked for */
    int32_t reserved;
    int64_t part_floats;    /* floats of split-KV scratch lent, 0: none (ace355_attention lends 16 Mi) */
} ace355_attn_request;
typedef struct ace355_attn_plan_info {
    int32_t kernel, nw;                          /* ACE355_ATTN_KERNEL_* and its template argument */
    int32_t grid_x, grid_y, grid_z, threads;
    int32_t kv_split;                            /* 1: one pass */
    int32_t merge_grid;                          /* workgroups of the merge launch that follows a split, 0: none */
    int32_t mx_out_ok;                           /* the kernel of this request can write MXFP8 */
} ace355_attn_plan_info;
int ace355_attn_plan(const ace355_attn_request* request, ace355_attn_plan_info* plan_out);
/* The same for the conv launches of the VAE (and ace355_conv1d_nlc): which instantiation of conv_kernel and which grid a request gets
 * under the process's ACE355_CONV_* switches.  The structs are the library's ConvRequest / ConvPlan (csrc/vae_plan.h), described there. */
typedef struct ace355_conv_request {
    int32_t B, M, N, Cin, taps;
    int32_t in_snake;       /* the launch applies a Snake while staging its input */
    int32_t x_view;         /* the input is the shifted flat view of a strided conv */
    int32_t res;            /* a residual is added */
    int32_t fused;          /* one-launch residual unit (the k = 1 conv inside the launch) */
    int32_t reserved;
} ace355_conv_request;
typedef struct ace355_conv_plan_info {
    int32_t bn, tm, ws;                          /* conv_kernel<bn = 32 | 128, tm = 128 | 256, ws = 0 | 1> */
    int32_t grid_x, grid_y, grid_z, threads;
    int32_t ras_tm, ras_tn;                      /* XCD-aware rasterisation of a (ras_tm x ras_tn) tile grid, 0: the plain grid */
    int32_t reserved;
} ace355_conv_plan_info;
int ace355_conv_plan(const ace355_conv_request* request, ace355_conv_plan_info* plan_out);

/* ------------------------------------------------------------------------------------------
 * DiT decoder (AceStepDiTModel, base.py:1240-1507) + sampler (generate_audio, base.py:1783-1989)
 * ---------------------------------------------------------------------------------------- */
typedef struct ace355_dit ace355_dit;

/* Fields of AceStepConfig the path uses (models/base/configuration_acestep_v15.py:148-263). */
typedef struct ace355_dit_config {
    int32_t hidden_size;       /* 2048 */
    int32_t intermediate_size; /* 6144 */
    int32_t num_layers;        /* 24 */
    int32_t num_heads;         /* 16 */
    int32_t num_kv_heads;      /* 8 */
    int32_t head_dim;          /* 128 (only 128 is supported) */
    int32_t sliding_window;    /* 128: |i-j| <= window, inclusive (base.py:99-105) */
    int32_t patch_size;        /* 2 (only 2 is supported) */
    int32_t in_channels;       /* 192 = 128 context + 64 latent */
    int32_t out_channels;      /* 64 */
    float rms_norm_eps;        /* 1e-6 */
    float rope_theta;          /* 1e6 */
    uint64_t sliding_layer_mask; /* bit i set = layer i is "sliding_attention" (cfg.py:251-254) */
} ace355_dit_config;

/* Replaces H/mlx_dit_init.py:9-43 (_init_mlx_dit) + models/mlx/dit_convert.py:69-84. */
int ace355_dit_create(const ace355_dit_config* cfg, ace355_dit** out);
void ace355_dit_destroy(ace355_dit* h);

/* Upload one tensor of AceStepDiTModel.state_dict() by its reference name (e.g.
 * "layers.3.self_attn.q_proj.weight", "proj_in.1.weight", "time_embed.linear_1.bias",
 * "scale_shift_table").  `data` holds `numel` elements of `dtype`, on host or device.
 * The library converts / packs into its own MFMA-friendly bf16 layout (fused QKV,
 * interleaved gate|up, patchify as GEMM).  Unknown names or wrong numel -> ERR_INVALID. */
int ace355_dit_load_tensor(ace355_dit* h, const char* name, const void* data, int dtype, int64_t numel, int is_device);
/* Verifies that every tensor was loaded; must be called once before set_condition/forward. */
int ace355_dit_finalize(ace355_dit* h);

/* Encoder conditioning for one "slot" (cond, null, non-cover cond, ...).
 * Runs condition_embedder (base.py:1359) and every layer's cross-attention
 * K = k_norm(k_proj(.)), V = v_proj(.) ONCE (the reference's EncoderDecoderCache,
 * base.py:312-329, 1875) and keeps them resident until the slot is overwritten.
 * enc: dev f32 [rows, hidden]; rows == L, or rows == 1 to broadcast one row over L keys
 * (null_condition_emb.expand_as, base.py:1907).  slot in [0, ACE355_MAX_SLOTS). */
int ace355_dit_set_condition(ace355_dit* h, int slot, const float* enc_dev, int rows, int L, void* stream);

/* One decoder forward = AceStepDiTModel.forward (base.py:1303-1507) with use_cache=True and
 * a filled cross cache.  x dev f32 [N,T,64]; ctx dev f32 [N,T,128]; t, t_r host [N];
 * slots host [N] (which condition slot each sequence attends to); v_out dev f32 [N,T,64]. */
int ace355_dit_forward(ace355_dit* h, const float* x_dev, const float* ctx_dev, const float* t_host,
                       const float* t_r_host, const int32_t* slots_host, int N, int T, float* v_out_dev, void* stream);

/* Cross-attention probabilities for lyric alignment: the reference's get_lyric_timestamp / get_lyric_score call the decoder with
 * output_attentions=True (handler/lyric_timestamp.py:78, lyric_score.py:97) and read the maps P = softmax_fp32(q k^T scale) of
 * eager_attention_forward (base.py:352) for a few (layer, head) pairs (custom_layers_config, acestep/handler.py:129).  Both padding
 * masks are discarded (base.py:1384-1385): every encoder row is attended.  Query head h reads KV head h / (Hq / Hkv) (repeat_kv).
 * Same inputs as ace355_dit_forward; pairs_host = n_pairs (layer, head) int32 pairs in strictly increasing order.  maps_out dev f32
 * [n_pairs][N][L][S] (S = ceil(T / 2)): attn_weights[n, head, s, j] of that layer, transposed to [L, S] as the handlers do.  The scores
 * are not rounded to bf16 before the softmax (the reference's GPU matmul does; its fp32 CPU path does not).
 * The forward stops after the maps of the last requested layer: that layer's attention and MLP and every later layer do not run (no map
 * depends on them; the reference runs them and discards the work, base.py:1454-1456).  Eager only (never captured); captured sampler
 * graphs stay valid.  Every precision; in ACE355_PRECISION_MXFP8 the maps carry that mode's projection numerics.
 * ERR_INVALID: a null pointer, n_pairs < 1, a layer outside [0, num_layers) or a head outside [0, num_heads), pairs unsorted or
 * duplicated, N outside [1, ACE355_MAX_SEQS], a slot not set or broadcast (rows == 1), slots of different L.  ERR_STATE: not finalized, a
 * stale slot (ace355_dit_set_adapters).  Nothing is enqueued on error. */
int ace355_dit_cross_attention_maps(ace355_dit* h, const float* x_dev, const float* ctx_dev, const float* t_host,
                                    const float* t_r_host, const int32_t* slots_host, int N, int T, const int32_t* pairs_host,
                                    int n_pairs, float* maps_out_dev, void* stream);

/* Knobs of generate_audio (base.py:1796-1812) that survive past prepare_condition. */
typedef struct ace355_sample_params {
    int32_t num_steps;          /* len(t_sched) - 1 */
    const float* t_sched_host;  /* [num_steps+1] fp32, base.py:1864-1867 (caller applies shift / custom timesteps) */
    float guidance_scale;       /* diffusion_guidance_sale; > 1 enables CFG batch doubling (base.py:1905) */
    float cfg_interval_start;   /* base.py:1945 */
    float cfg_interval_end;
    int32_t infer_method;       /* 0 = "ode" (base.py:1974-1979); 1 = "sde" (base.py:1968-1973), needs sde_noise_dev */
    int32_t use_adg;            /* 1 = angle-based guidance (apg_guidance.py:107-180) instead of APG inside the cfg interval */
    int32_t cond_slot;          /* slot of the cover/main condition */
    int32_t null_slot;          /* slot holding null_condition_emb (ignored when guidance <= 1) */
    int32_t cover_switch_step;  /* = int(steps * audio_cover_strength); >= num_steps: never switch (base.py:1916-1927) */
    int32_t non_cover_slot;     /* slot + context used from cover_switch_step on */
    const float* ctx_non_cover_dev; /* dev f32 [B,T,128] or NULL */
    const float* sde_noise_dev;     /* "sde" only: dev f32 [num_steps,B,T,64], the per-step randn_like(x) draws of base.py:1777
                                     * (the reference draws them unseeded on the model device; the caller owns the RNG) */
    /* Per-item conditions inside one call: the reference's loop takes B distinct encoder_hidden_states rows
     * (base.py:1905-1911, switch :1916-1927).  host int32 [B] each, or NULL = every item uses cond_slot / non_cover_slot.
     * All slots of one call must hold the same encoder length L. */
    const int32_t* cond_slots_host;
    const int32_t* non_cover_slots_host;
    int32_t sde_next_from_sched;    /* "sde" renoise level after step i: 0 = 1 - (i+1)/num_steps (base / sft, base.py:1972);
                                     * 1 = t_sched[i+1] (turbo model, models/turbo/modeling_acestep_v15_turbo.py:1980-1984) */
} ace355_sample_params;

/* The sampling loop of generate_audio (base.py:1913-1981): CFG doubling, steps x {decoder forward,
 * APG (apg_guidance.py:33-56, momentum -0.75, norm threshold 2.5, fp64 projection), Euler update}.
 * xt0 dev f32 [B,T,64] is the initial state (noise, or the cover renoise of base.py:1887, prepared by
 * the caller on the host with the CPU generator: SURVEY.md section 7.2 "Noise parity");
 * ctx dev f32 [B,T,128]; latents_out dev f32 [B,T,64] ("target_latents").
 * per_step_ms_host (optional, [num_steps]) receives HIP-event step times. */
int ace355_dit_sample(ace355_dit* h, const float* xt0_dev, const float* ctx_dev, int B, int T,
                      const ace355_sample_params* p, float* latents_out_dev, float* per_step_ms_host, void* stream);

/* Compute precision of the four big projections of every layer (QKV, o_proj, gate|up, down).  BF16 (default) = the reference GPU
 * path's dtype.  MXFP8 = BASELINE configs[4] "fp8 MFMA": OCP MXFP8 operands (e4m3, one E8M0 scale per 32 K elements; weights
 * quantised once here, activations per launch) on v_mfma_scale_f32_32x32x64_f8f6f4, fp32 accumulate, same epilogues; launches with
 * fewer than 1536 token rows keep the bf16 kernels.  The reference's counterpart is torchao fp8 on the DiT Linears
 * (handler/init_service_loader.py:89-113; absent here: parity unpinned, tolerance stated in DESIGN.md).  Call after finalize.
 * FP8_WEIGHT_ONLY = the reference's default fp8 knob (`quantization="fp8_weight_only"`, torchao Float8WeightOnlyConfig,
 * init_service_loader.py:95-97): weights as e4m3 with one fp32 scale per output channel, activations and arithmetic bf16.  gfx950 has
 * no bf16 x fp8 MFMA, so this mode applies the NUMERICS (every Linear weight rounded through per-channel e4m3 once, in place) and
 * runs the bf16 kernels: same speed and memory as BF16.  One way: load the weights again to go back. */
#define ACE355_PRECISION_BF16 0
#define ACE355_PRECISION_MXFP8 1
#define ACE355_PRECISION_FP8_WEIGHT_ONLY 2
int ace355_dit_set_precision(ace355_dit* h, int precision);

/* hipGraph replay of the sampling loop: with enable != 0, ace355_dit_sample captures its launch
 * sequence (steps x ~360 kernels) into a graph on first use and replays it for every later call with the same shapes, schedule,
 * knobs, slot layout and stream; any change re-captures.  Results are identical to the eager path of the same chain configuration (same
 * kernels, same order; by default a captured call runs as ONE sampler chain - two chains become two graph branches that the runtime
 * places on streams of its own choosing, measured slower - while an eager request of 2-3 songs runs as two: ace355_dit_set_dual).
 * Off by default; ACE355_SAMPLE_GRAPH=1 in the environment turns it on at handle creation.  graph_stats: captures / replays so far. */
int ace355_dit_set_graph(ace355_dit* h, int enable);
int ace355_dit_graph_stats(ace355_dit* h, int64_t* captures, int64_t* replays);

/* RMSNorm folding (on by default; ACE355_NORM_FOLD=0 in the environment or enable = 0 here turns it off): in bf16 ace355_dit_sample calls
 * of >= 64 token rows (ACE355_NORM_FOLD_MIN_ROWS; since round 3 it pays at every real size) the three RMSNorms of a decoder layer
 * (base.py:493-533) are not kernels of their own: the residual GEMM that finishes hidden_states also writes bf16(h * g) and the rows' sums of
 * squares, the consuming projection applies rsqrt(mean(h^2) + eps) and the modulation shift's projection (shift W^T, precomputed per step of
 * the schedule at the start of the call) to its fp32 accumulators.  Same math, one bf16 rounding placed differently.  A row's sum of squares
 * is gathered per aligned 128-column group - (b0 + b1) + (b2 + b3) over its four 32-column blocks in fp32, then 2^-24 fixed point and integer adds -
 * so it does not depend on the GEMM tile form a row was computed in (round 6).
 * enable: 0 off, 1 default, 2 every call the kernels support whatever its size (tests). */
int ace355_dit_set_norm_fold(ace355_dit* h, int enable);

/* Dual-chain sampler.  The songs of a request are independent through the whole sampling loop of generate_audio (per-item noise,
 * per-item CFG / APG; base.py:1783-1989), so a call with B >= 2 songs can run as TWO half-batch samplers - songs [0, ceil(B/2)) on the
 * caller's stream, the rest on a side stream that sits on a hardware queue of its own (checked once per caller stream: the runtime
 * shares a few queues between all streams, and two streams on one queue run strictly in turn).  mode 0: one chain; 1 (default,
 * ACE355_DUAL): two chains when one chain's launches would under-fill the chip: <= 2400 token rows in the whole request
 * (ACE355_DUAL_MAX_ROWS: 2-3 songs of 30 s under CFG), or a row count whose tiles leave more than 15 % of the CU slots of their
 * rounds empty (30 s songs: 5, 6, 9, 10 per request; not 4, 7, 8) - there one chain's launches fill the CUs the other leaves idle (per
 * request incl. decode, one chain -> two: 2 x 30 s 199 -> 194 ms, 3: 266 -> 251, 5: 397 -> 358, 6: 430 -> 409, 9: 658 -> 582);
 * 2: two chains whenever B >= 2 (4 songs: 290 -> 304 ms, the metric batch of 8: 487 -> 519 ms: one chain already gives every CU a
 * tile and the two chains only share the power cap).  Each song's
 * result is what a one-chain call with that song's half-batch returns.  Captured like any other launch under ace355_dit_set_graph.
 * dual_count: calls that ran as two chains so far. */
int ace355_dit_set_dual(ace355_dit* h, int mode);
int ace355_dit_dual_count(ace355_dit* h, int64_t* calls);

/* Layer-0 de-duplication under classifier-free guidance (on by default; ace355_dit_set_dedup(h, 0) or ACE355_DEDUP0=0 in the environment switch it off).  The
 * reference feeds the decoder x = cat([xt, xt]) with the same context latents and timestep for both copies (base.py:1905-1911, 1929): up to
 * the first cross-attention (base.py:499-511 of layer 0) the conditional and the null copy of a song are the same numbers.
 * ace355_dit_sample therefore runs layer 0's first norm, QKV projection and self-attention on the conditional half only and lets the
 * o_proj GEMM read that half's attention output for both halves.  dedup_count: forwards that took the shortcut so far - counted when a
 * forward is ENQUEUED: replays of a captured sampler graph (ace355_dit_set_graph) run the shortcut without advancing it. */
int ace355_dit_set_dedup(ace355_dit* h, int enable);
int ace355_dit_dedup_count(ace355_dit* h, int64_t* forwards);

/* LoRA adapters, merged into the packed weights (PEFT LoraLayer semantics: the unmerged eval forward y = x W^T + scaling (x A^T) B^T
 * equals a forward with W + scaling B A; the reference loads, removes, toggles and scales adapters in H/lora/lifecycle.py and
 * H/lora/controls.py).  One term = one adapter on one target weight.  `name` is the reference key of the target, one of the ten
 * kinds per layer: layers.{i}.{self_attn,cross_attn}.{q,k,v,o}_proj.weight and layers.{i}.mlp.{gate,up,down}_proj.weight;
 * A_dev = lora_A.weight [rank, in], B_dev = lora_B.weight [out, rank], bf16 row-major, on the device (the reference casts them to
 * the model dtype, .to(self.dtype)); scale = PEFT scaling[adapter] (alpha / r, or alpha / sqrt(r) with use_rslora) x the user's
 * scale (H/lora/controls.py:83-113). */
typedef struct ace355_lora_term {
    const char* name;
    const void* A_dev;
    const void* B_dev;
    int32_t rank;
    float scale;
} ace355_lora_term;
/* Replace the WHOLE adapter state: afterwards every target weight is bf16_rne(float(W0) + sum_j s_j B_j A_j) (fp32 products, each
 * term scaled in fp32, one rounding) and every other weight is W0, whatever the earlier calls were.  Several terms may name one target;
 * terms with scale 0 are dropped (scale 0 gives the base bits); n_terms 0 restores the base.  The merge runs on `stream`, in place:
 * weight addresses never change, so chain contexts, prefetch plans and captured sampler graphs (which replay with the new weights) stay
 * valid.  The call is synchronous: it synchronises `stream` before it uploads its tables and again after the merge, so A / B may be
 * released when it returns.  A target's base rows are kept in a pristine copy from the first merge that touches them until no adapter
 * is left.
 * Needs a finalized handle in ACE355_PRECISION_BF16 whose weights did not go through the fp8 round trip (the reference refuses LoRA on
 * quantised models, H/lora/lifecycle.py:173-178): ERR_STATE otherwise.  An unknown name, rank < 1 or a null pointer: ERR_INVALID.
 * While adapters are applied, ace355_dit_set_precision to another precision and ace355_dit_load_tensor return ERR_STATE.  A call
 * that rewrites a cross-attention k / v (or o, for broadcast slots) projection makes the condition slots built before it stale:
 * a forward / sample reading one returns ERR_STATE until ace355_dit_set_condition rebuilds it.
 * Which launches a call makes: ace355_adapter_plan. */
int ace355_dit_set_adapters(ace355_dit* h, const ace355_lora_term* terms, int n_terms, void* stream);
/* LoKr adapters (LyCORIS LokrModule semantics, restated from its published source: the weight delta of a module is
 * scale x multiplier x kron(W1, W2), each factor held in full or as a low-rank product w_a @ w_b).  The reference loads a LoKr
 * artefact through LyCORIS (H/lora/lifecycle.py:16-155, 232-236) and toggles / scales it with set_multiplier
 * (H/lora/controls.py:12-32, 49-55, 121-129).  One term on a target [out, in] with out = out_l out_k, in = in_m in_n:
 *     dW[l out_k + k, m in_n + n] = scale W1[l, m] W2[k, n],
 *     W1 = w1 [out_l, in_m] or w1a [out_l, r1] @ w1b [r1, in_m],   W2 = w2 [out_k, in_n] or w2a [out_k, r2] @ w2b [r2, in_n].
 * All factor tensors are bf16, row-major, on the device (the reference casts the decoder, LyCORIS modules included, to the model
 * dtype: lifecycle.py:251).  `name` is one of the ten target kinds of ace355_lora_term. */
typedef struct ace355_kron_term {
    const char* name;                       /* same ten target kinds as ace355_lora_term */
    const void *w1_dev, *w1a_dev, *w1b_dev; /* exactly one of {w1} / {w1a, w1b} set */
    const void *w2_dev, *w2a_dev, *w2b_dev; /* exactly one of {w2} / {w2a, w2b} set */
    int32_t out_l, out_k, in_m, in_n, r1, r2;   /* r1 / r2 = 0 for a full factor */
    float scale;
} ace355_kron_term;
/* ace355_dit_set_adapters for a state that mixes both families: replaces the WHOLE adapter state, with the same synchrony,
 * pristine-copy lifetime, stale-slot marking and precision refusals.  Every rewritten weight is bf16_rne(float(W0) + sum_j dW_j):
 * a decomposed factor's product is formed in fp32 (rank order) in a scratch table of the handle, the Kronecker products and the
 * sum over a target's terms (call order) are fp32, one rounding.  n_kron 0 IS ace355_dit_set_adapters (the same launches, the same
 * bits).  Several Kronecker terms may name one target; scale 0 drops a term.  ERR_INVALID: a target named by both a LoRA and a
 * Kronecker term (the reference never has both, lifecycle.py:244-246), out_l out_k != out or in_m in_n != in, a missing or doubled
 * factor pointer (a full factor has rank 0, a decomposed one rank >= 1), a rank below 0, a non-finite scale, an unknown name.
 * Which launches a call makes: ace355_adapter_plan. */
int ace355_dit_set_adapters_mixed(ace355_dit* h, const ace355_lora_term* lora, int n_lora, const ace355_kron_term* kron, int n_kron,
                                  void* stream);
/* DoRA (weight decomposition) on top of the additive terms of one target: LyCORIS LokrModule with `wd` (forward, not bypass:
 * apply_weight_decompose) and PEFT LoRA with use_dora.  Neither library is part of the reference tree; the semantics are restated from
 * their published modules and are unpinned.  With V = float(W0) + sum_j dW_j, the fp32 value ace355_dit_set_adapters_mixed forms
 * before its single rounding (the terms in call order, their scales holding the multiplier),
 *     n  = ||V||_2 over the row (per_input 0: one n, one g per output row) or over the column (per_input 1: per input column),
 *     f  = 1 + m (g / (n + eps) - 1),        W' = bf16_rne(V f).
 * LyCORIS: g = dora_scale ([out, 1]: per_input 0, [1, in]: per_input 1), m = multiplier, eps = finfo(dora_scale.dtype).eps (2^-7 for
 * the bf16 the reference casts its decoder to).  PEFT: g = lora_magnitude_vector [out], per_input 0, eps 0, m 1.  Where n + eps == 0
 * (PEFT, an all-zero row) f = 1: a documented deviation, PEFT would produce NaN.
 * Arithmetic: V in fp32 exactly as the plain merge forms it.  The sum of squares accumulates in fp64 from the fp32 values of V, in a
 * fixed order and without atomics: inside a 64 x 128 merge tile a thread's 8 columns (axis "out") or 4 rows (axis "in") in index order,
 * then the lanes and waves of the tile in a fixed tree, then the tiles of the row or column in tile order.  n = sqrt(sum) and f are
 * formed in fp64 and f is rounded to fp32 once; V f is one fp32 product followed by one bf16 rounding.  g_dev holds fp32 values on the
 * device, n = out (per_input 0) or in (per_input 1) of them, indexed by the reference row / column whatever the packed layout; the
 * caller converts them from the values the reference holds (after its cast to the model dtype).  Bit-reproducible call to call. */
typedef struct ace355_dora_term {
    const char*  name;       /* same ten target kinds as ace355_lora_term */
    const float* g_dev;      /* out (per_input 0) or in (per_input 1) fp32 values on the device */
    int32_t      per_input;  /* 0 | 1 */
    float        eps;        /* >= 0 */
    float        multiplier; /* m; 0 drops the term (f = 1: the additive terms alone, which the reference gives scale 0 then too) */
} ace355_dora_term;
/* ace355_dit_set_adapters_mixed plus at most one DoRA term per target: replaces the WHOLE adapter state, with the same synchrony,
 * pristine-copy lifetime, stale-slot marking, precision refusals and invalidation of the folded-norm tables.  A target with a DoRA
 * term runs twice through its merge kernel on `stream` (partial sums of squares into a scratch of the handle that grows on demand and
 * is freed with it, then the rescaled write); targets without one keep the single-pass launches and the bits of
 * ace355_dit_set_adapters_mixed.  n_dora 0 IS ace355_dit_set_adapters_mixed (the same launches, the same bits).  g_dev may be released
 * when the call returns.  ERR_INVALID, nothing changed: two DoRA terms on one target, a DoRA term with multiplier != 0 on a target
 * that no LoRA / Kronecker term of the call names, a null g_dev, per_input outside {0, 1}, a non-finite or negative eps, a non-finite
 * multiplier, an unknown name, and everything ace355_dit_set_adapters_mixed refuses.  Which launches a call makes: ace355_adapter_plan. */
int ace355_dit_set_adapters_dora(ace355_dit* h, const ace355_lora_term* lora, int n_lora, const ace355_kron_term* kron, int n_kron,
                                 const ace355_dora_term* dora, int n_dora, void* stream);
/* Which targets, tables, scratch regions and launches a set_adapters call comes to (no reference counterpart; a test and review aid, as
 * ace355_gemm_plan): the three entry points above do exactly what one pure function of the call says (csrc/adapter_plan.h
 * plan_adapters), and this evaluates it for a decoder of configuration `cfg` whose targets `applied` (n_applied names) hold a merge now.
 * No GPU is touched and no handle is needed; the device pointers of the terms are only tested (null, and w2 for 16-byte alignment) and
 * may be any numbers.  Refusals are those of the entry points, code and message; a name among `applied` that is no target is
 * ERR_INVALID.  Every array of `rows` is caller-sized: up to its cap rows are written, `info` holds the full counts. */
#define ACE355_ADAPTER_CLASS_LORA 0       /* plain, formed by the LoRA merge kernel (and, in a call without a live Kronecker term, restored) */
#define ACE355_ADAPTER_CLASS_KRON 1       /* plain, formed by the Kronecker merge kernel (and, beside a live Kronecker term, restored) */
#define ACE355_ADAPTER_CLASS_DORA_LORA 2  /* DoRA, V formed by the LoRA merge kernel */
#define ACE355_ADAPTER_CLASS_DORA_KRON 3  /* DoRA, V formed by the Kronecker merge kernel */
#define ACE355_ADAPTER_KERNEL_LORA_MERGE 0
#define ACE355_ADAPTER_KERNEL_KRON_FACTORS 1
#define ACE355_ADAPTER_KERNEL_KRON_MERGE 2
#define ACE355_ADAPTER_KERNEL_DORA_FACTORS 3
#define ACE355_ADAPTER_SECTIONS 9 /* of the device table: LoRA targets, LoRA terms, Kronecker targets, Kronecker terms, factor jobs, DoRA-LoRA
                                   * targets, their DoRA rows, DoRA-Kronecker targets, their DoRA rows */
typedef struct ace355_adapter_target_info {
    const char* name;            /* the caller's string */
    int32_t cls;                 /* ACE355_ADAPTER_CLASS_*: which launches it rides */
    int32_t row;                 /* its row in its class's target section; in a DoRA class also its row among the class's DoRA rows */
    int32_t rows, cols;
    int32_t tile0, tiles_n;      /* first tile in its class's launches, column tiles per row tile */
    int32_t term0, nterms;       /* its rows of the LoRA resp. Kronecker term section */
    int32_t restored;            /* 1: no term now, its rows go back to the base */
} ace355_adapter_target_info;
typedef struct ace355_adapter_launch_info {
    int32_t kernel, pass;        /* ACE355_ADAPTER_KERNEL_*; pass 0 plain, 1 / 2 the DoRA passes of a merge kernel */
    int32_t entries;             /* rows of its first section */
    int32_t grid_x, grid_y, lds_bytes;
    int32_t sections[3];         /* table sections it reads, -1: none */
} ace355_adapter_launch_info;
typedef struct ace355_adapter_kron_info {   /* one row of the Kronecker term section */
    int32_t out_l, out_k, in_m, in_n, wide, w1_f32, w2_f32;
    float scale;
    int64_t w1_offset, w2_offset; /* bytes into the factor scratch where the factor is a product (w*_f32), else -1 */
} ace355_adapter_kron_info;
typedef struct ace355_adapter_factor_info { /* one row of the factor job section */
    int32_t rows, cols, rank, tile0, tiles_n, reserved;
    int64_t offset;              /* bytes into the factor scratch */
} ace355_adapter_factor_info;
typedef struct ace355_adapter_dora_info {   /* one DoRA row; cls 2 rows first, then cls 3, each in target order */
    int32_t cls, per_input, n, ntiles;
    float eps, multiplier;
    int64_t part_offset, f_offset; /* bytes into the DoRA scratch */
} ace355_adapter_dora_info;
typedef struct ace355_adapter_plan_rows {
    ace355_adapter_target_info* targets;  int32_t cap_targets;
    ace355_adapter_launch_info* launches; int32_t cap_launches;
    ace355_adapter_kron_info* kron;       int32_t cap_kron;
    ace355_adapter_factor_info* factors;  int32_t cap_factors;
    ace355_adapter_dora_info* dora;       int32_t cap_dora;
} ace355_adapter_plan_rows;
typedef struct ace355_adapter_plan_info {
    int32_t n_targets, n_merged;  /* merged targets first, in first-mention order, then the restored ones */
    int32_t n_launches, n_lora_terms, n_kron_terms, n_factors, n_dora;
    int32_t stale_kv, stale_o;    /* the call makes condition slots built from the cross-attention k / v resp. o weights stale */
    int32_t reserved;
    int64_t table_bytes, kscratch_floats, dscratch_bytes;
    int64_t section_at[ACE355_ADAPTER_SECTIONS], section_bytes[ACE355_ADAPTER_SECTIONS];
} ace355_adapter_plan_info;
int ace355_adapter_plan(const ace355_dit_config* cfg, const ace355_lora_term* lora, int n_lora, const ace355_kron_term* kron, int n_kron,
                        const ace355_dora_term* dora, int n_dora, const char* const* applied, int n_applied,
                        const ace355_adapter_plan_rows* rows, ace355_adapter_plan_info* info);
/* Copy the live (merged) weight of one of the ten target kinds above to dst_dev in the reference layout [out, in] (the inverse of the
 * packing's row map), as ACE355_DTYPE_F32 or ACE355_DTYPE_BF16; enqueued on `stream`.  Tests, and export of merged weights. */
int ace355_dit_read_weight(ace355_dit* h, const char* name, void* dst_dev, int dtype, void* stream);

/* Test / debug hook: after decoder layer `layer` (0-based) of every following forward, copy the fp32 residual stream
 * hidden_states [N*S, hidden] (the layer's output, base.py:539) to dst_dev; dst_dev NULL clears the tap.  Lets the parity
 * tests compare the per-layer activations the golden fixtures hold, not only the final velocity. */
int ace355_dit_set_tap(ace355_dit* h, int layer, float* dst_dev);

/* Asynchronous device-side conditions of the calls queued so far on `stream` (synchronises it): today the ordered split-K of the
 * small-M residual GEMMs, whose parts wait for their turn with a bound - a missed turn is counted on the device, reported here as
 * ACE355_ERR_HIP and the turn counters are reset.  ACE355_OK otherwise.  The Python host calls it where it synchronises anyway. */
int ace355_dit_poll_errors(ace355_dit* h, void* stream);
/* Release the cross-K/V buffers of condition slots [first_unused, ACE355_MAX_SLOTS) (a request with many distinct conditions
 * leaves up to 32 x 150 MB resident otherwise).  Synchronises the device when there is something to free. */
int ace355_dit_trim_slots(ace355_dit* h, int first_unused);
/* Work counters for roofline accounting: algorithmic FLOPs of the last forward (SURVEY.md section 8d formula)
 * and GEMM-only HIP-event time when profiling was enabled with ace355_dit_set_profile(h, 1). */
int ace355_dit_set_profile(ace355_dit* h, int enable);
int ace355_dit_get_profile(ace355_dit* h, double* gemm_ms, double* gemm_flops, double* attn_ms, double* attn_flops,
                           int64_t* gemm_launches);

/* One decoder pass (ace355_dit_forward, a step of ace355_dit_sample, ace355_dit_cross_attention_maps) as data, in launch order:
 * plan_dit_pass of csrc/dit_plan.h, which the handle executes step by step.  A step names everything its launch takes except pointers
 * and the sampler's step index; buffers appear as roles.  No GPU, no handle. */
#define ACE355_DIT_STEP_MOD_GS 0        /* the (g, shift) vectors of the 2 NL modulated norms for this call's timestep rows */
#define ACE355_DIT_STEP_ZERO_ROWSQ 1    /* zero fill of the folded norms' row sums (count elements) */
#define ACE355_DIT_STEP_NORM_GS 2       /* rmsnorm(h) g + shift of table entry gs -> bf16 rows (dst) */
#define ACE355_DIT_STEP_NORM_GS_MX 3    /* ... -> MXFP8 rows */
#define ACE355_DIT_STEP_NORM_W 4        /* the cross-attention norm (plain weight) -> bf16 rows */
#define ACE355_DIT_STEP_NORM_W_MX 5     /* ... -> MXFP8 rows */
#define ACE355_DIT_STEP_GEMM 6
#define ACE355_DIT_STEP_TRANSPOSE_V 7
#define ACE355_DIT_STEP_ATTN_SELF 8
#define ACE355_DIT_STEP_ATTN_CROSS 9
#define ACE355_DIT_STEP_XATTN_PROBS 10
#define ACE355_DIT_STEP_TAP 11          /* ace355_dit_set_tap's copy of the residual stream (count elements) */
#define ACE355_DIT_STEP_NORM_OUT 12     /* norm_out with the timestep embedding's shift / scale */
#define ACE355_DIT_PROJ_PATCHIFY 0
#define ACE355_DIT_PROJ_QKV 1
#define ACE355_DIT_PROJ_O 2
#define ACE355_DIT_PROJ_CROSS_Q 3
#define ACE355_DIT_PROJ_CROSS_O 4
#define ACE355_DIT_PROJ_GATE_UP 5
#define ACE355_DIT_PROJ_DOWN 6
#define ACE355_DIT_PROJ_OUT 7
#define ACE355_DIT_PATH_BF16 0
#define ACE355_DIT_PATH_MX_QUANT 1      /* the bf16 operand is block-quantised first, then the MXFP8 GEMM */
#define ACE355_DIT_PATH_MX 2            /* the MXFP8 GEMM on an operand its producer left as MXFP8 (src xq or aq) */
#define ACE355_DIT_BUF_NONE (-1)
#define ACE355_DIT_BUF_XIN 0            /* packed patch input bf16 [N][2S][in_channels] */
#define ACE355_DIT_BUF_H 1              /* residual stream f32 [M][D] */
#define ACE355_DIT_BUF_XN 2             /* normed rows bf16 [M + 1][D] */
#define ACE355_DIT_BUF_QKV 3            /* q | k | v rows (self), q rows (cross) */
#define ACE355_DIT_BUF_AO 4             /* attention output bf16 [M + 1][QD] */
#define ACE355_DIT_BUF_ACT 5            /* SwiGLU output bf16 [M + 1][F] */
#define ACE355_DIT_BUF_AQ 6             /* SwiGLU output as MXFP8 */
#define ACE355_DIT_BUF_XQ 7             /* the MXFP8 operand scratch */
#define ACE355_DIT_BUF_VT 8             /* V^T [N][KVH][128][Sp] */
#define ACE355_DIT_BUF_VPAD 9           /* velocity rows f32 [M][2 out_channels] */
#define ACE355_DIT_BUF_SLOT_KV 10       /* the condition slots' K rows / V^T tables, per sequence */
#define ACE355_DIT_BUF_TAP 11
#define ACE355_DIT_BUF_MAPS 12
#define ACE355_DIT_G_NORM_CA (-2)       /* nf_gA: the layer's cross_attn_norm weight instead of a (g, shift) table entry */
typedef struct ace355_dit_pass_request {
    int32_t N, T;
    int32_t temb_rows;                       /* 1: every sequence shares one timestep (the sampler); else N */
    int32_t seq_slot[ACE355_MAX_SEQS];       /* per sequence: its condition slot ... */
    int32_t seq_L[ACE355_MAX_SEQS];          /* ... that slot's key count (0: the slot is not set) ... */
    int32_t seq_broadcast[ACE355_MAX_SEQS];  /* ... and whether it was set from one row (rows == 1) */
    int32_t precision;                       /* ACE355_PRECISION_BF16 / _MXFP8 (the compute path) */
    int32_t mx_min_rows;                     /* token rows below which MXFP8 launches stay bf16 (1536) */
    int32_t mx_copies;                       /* MXFP8 weight copies that exist: 1 qkv, 2 o, 4 gate|up, 8 down, 16 cross q, 32 cross o; -1: those
                                                ace355_dit_set_precision makes for the configuration */
    int32_t nf_on, nf_emb_on, nf_rows;       /* the sampler call runs folded / reads its embeddings from the schedule tables / their steps */
    int32_t dup_half;                        /* sequences [N/2, N) enter with the inputs of [0, N/2) (a CFG sampler step) */
    int32_t dedup_on;                        /* ace355_dit_set_dedup */
    int32_t prefetch;                        /* weight prefetch allowed (one chain) */
    int32_t cu_slots;                        /* 0: the whole chip; 128: a chain planned for half of it */
    int32_t graph_mode;                      /* ace355_dit_set_graph */
    int32_t zr_M;                            /* the row of xn / ao / act the handle last zeroed, -1: none */
    int32_t map_last;                        /* cross-attention maps: the last layer with a request (the pass stops there), -1: no maps */
    int32_t map_heads[64];                   /* ... and the number of requested heads per layer */
    int32_t qkv_vt_epilogue;                 /* GemmPlan::vt_epilogue of the QKV launch at M rows ... */
    int32_t qkv_vt_epilogue_half;            /* ... and at the conditional half's rows (layer 0 of a deduplicated CFG step) */
    int32_t self_mx_out_ok, cross_mx_out_ok; /* AttnPlan::mx_out_ok of the self- / cross-attention request */
    int64_t nf_cap_M;                        /* rows the row-sum table holds */
    uint64_t tap_mask;                       /* bit l: layer l is tapped (ace355_dit_set_tap) */
} ace355_dit_pass_request;
typedef struct ace355_dit_step_info {
    int32_t kind, layer;                     /* ACE355_DIT_STEP_*; -1 outside the layers */
    int32_t src, dst;                        /* ACE355_DIT_BUF_*: the row operand read, the buffer written */
    int32_t M;                               /* rows: GEMM M, rows a norm writes, mod_gs timestep rows */
    int32_t seqs;                            /* sequences of a transpose_v, attention or xattn_probs launch */
    /* GEMM: GemmEpilogue (csrc/common.h) without pointers */
    int32_t proj, path;                      /* ACE355_DIT_PROJ_*, ACE355_DIT_PATH_* */
    int32_t N, K, lda, ldw, ldc, mode;
    int32_t rows_per_seq;
    int32_t bias;                            /* the projection has a bias vector (patchify, proj_out) */
    int32_t gate;                            /* mode 2: row of the layer's scale_shift_table / of the timestep projection; -1: gate 1 */
    int32_t cvec, cvec_row0;                 /* rows >= cvec_row0 add the broadcast slot's constant (cvec 1) */
    int32_t hn;                              /* head-norm epilogue: 0 none, 1 self (q, k, RoPE), 2 cross (q only, no RoPE) */
    int32_t hn_q_cols, hn_qk_cols;
    int32_t vt_offered;                      /* V^T is offered to the epilogue */
    int32_t nf_split, nf_gA, nf_gB;          /* fold producer (nf_split >= 0): (g, shift) table entries or ACE355_DIT_G_NORM_CA ... */
    int32_t nf_sqA, nf_sqB;                  /* ... and row-sum table indices (3 layer + which) */
    int32_t nc_rowsq, nc_bias;               /* fold consumer (nc_rowsq >= 0): row-sum index; bias table 0 none, 1 qkv, 2 gate|up */
    int32_t a_wrap, a_zero_idx;
    int32_t mxo;                             /* the SwiGLU epilogue writes MXFP8 */
    int32_t next_proj, next_layer, next_M, next_N, next_K, next_mode;   /* prefetch target, next_proj -1: none */
    /* norms */
    int32_t gs;                              /* (g, shift) table entry: 2 layer + {0 self-attention, 1 MLP} */
    /* attention, xattn_probs */
    int32_t Sq, Skv, window, mx_out, Lpad;
    int32_t n_heads, pair0;                  /* xattn_probs: requested heads of the layer, index of its first pair in the output */
    int32_t reserved;
    int64_t count;
    double flops;
} ace355_dit_step_info;
typedef struct ace355_dit_pass_info {
    int32_t S, M, Sp, Nc, Mc, n_sc, L, Lpad;
    int32_t fold, emb, dedup0;
    int32_t zero_rows;                       /* the call zeroes row M of xn / ao / act first */
    int32_t n_steps, gemm_launches;
    int64_t vt_elems;                        /* bf16 elements of V^T the call zeroes when (N, S) changed */
    double gemm_flops, attn_flops;           /* sums over the steps */
} ace355_dit_pass_info;
/* cfg as ace355_dit_create checks it.  The four answers of other plans (qkv_vt_epilogue .. cross_mx_out_ok) are resolved here through
 * ace355_gemm_plan's and ace355_attn_plan's queries, so the steps are what a handle in that state would launch; those four fields of
 * `request` are ignored.  A refusal is ACE355_ERR_INVALID with forward's text.  steps_out may be NULL or shorter than the plan. */
int ace355_dit_pass_plan(const ace355_dit_config* cfg, const ace355_dit_pass_request* request, ace355_dit_step_info* steps_out,
                         int capacity, int32_t* n_out, ace355_dit_pass_info* info_out);

/* ------------------------------------------------------------------------------------------
 * Oobleck VAE decoder (diffusers AutoencoderOobleck.decode; restated in models/mlx/vae_model.py:190-230)
 * ---------------------------------------------------------------------------------------- */
typedef struct ace355_vae ace355_vae;

typedef struct ace355_vae_config {
    int32_t decoder_channels;       /* 128 */
    int32_t decoder_input_channels; /* 64 */
    int32_t audio_channels;         /* 2 */
    int32_t num_blocks;             /* 5 */
    int32_t channel_multiples[ACE355_MAX_BLOCKS]; /* [1,2,4,8,16] */
    int32_t upsampling_ratios[ACE355_MAX_BLOCKS]; /* decoder order, e.g. [10,6,4,4,2] (product = hop 1920) */
} ace355_vae_config;

/* Replaces H/mlx_vae_init.py:12-96 (_init_mlx_vae) + models/mlx/vae_convert.py. */
int ace355_vae_create(const ace355_vae_config* cfg, ace355_vae** out);
void ace355_vae_destroy(ace355_vae* h);
/* Names are AutoencoderOobleck.state_dict() keys, "decoder.*" and (optional) "encoder.*".  Which of them a handle needs, with which
 * element counts, is one table: vae_weight_table (csrc/vae_plan.h), one row per conv ("<base>.weight_g|weight_v", "<base>.bias") and per
 * Snake ("<base>.alpha|beta").  Any other key under the two prefixes is accepted and dropped.  Weight-norm is fused at finalize
 * (w = g*v/(||v||+1e-9), vae_convert.py:18-34); a pre-fused "<base>.weight" is taken in place of the pair.
 * ace355_vae_finalize checks every name and size first (ACE355_ERR_STATE "missing tensor", ACE355_ERR_INVALID "wrong size"; nothing is
 * touched then), builds the packed weights and CONSUMES the loaded tensors: a tensor loaded afterwards un-finalizes the handle, and the
 * next finalize needs the whole state dict again. */
int ace355_vae_load_tensor(ace355_vae* h, const char* name, const void* data, int dtype, int64_t numel, int is_device);
int ace355_vae_finalize(ace355_vae* h);
/* Replaces vae.decode(z).sample at H/vae_decode_chunks.py:42,95 / H/generate_music_decode.py:172-177 and
 * _mlx_vae_decode (H/mlx_vae_decode_native.py:31-72).  z dev f32 [B,64,T] (the reference's
 * [B,C,T] layout); wav_out dev f32 [B,2,hop*T].  Whole-sequence decode when the three activation buffers fit the decode
 * budget: equals the reference's overlap-discard tiling away from fp summation order.  Above the
 * budget the call splits itself: fewer items per pass first (exact), then overlap-discard windows in time whose halo covers
 * the decoder's receptive field (bit-identical to the whole-sequence result); a refused allocation halves the budget and
 * re-plans instead of failing (the reference's policy: H/memory_utils.py:48-83, H/vae_decode_chunks.py:40-112). */
int ace355_vae_decode(ace355_vae* h, const float* z_dev, int B, int T, float* wav_out_dev, void* stream);
/* Decode memory policy.  bytes > 0: budget of the three ping-pong activation buffers (default 96 GiB, or ACE355_VAE_BUDGET_MB at
 * create); overlap_frames > 0: halo per window side in latent frames (multiple of 8, >= the receptive field; default
 * max(16, receptive field + 2); the reference uses 64, H/vae_decode.py:16).  Zero leaves a setting unchanged. */
int ace355_vae_set_decode_budget(ace355_vae* h, int64_t bytes, int overlap_frames);
/* The window plan ace355_vae_decode would use for (B, T): items per window, core frames per window (== T: whole sequence),
 * halo frames, bytes of the three activation buffers.  Any output pointer may be NULL. */
int ace355_vae_decode_plan(ace355_vae* h, int B, int T, int32_t* items_per_window, int32_t* core_frames, int32_t* overlap_frames,
                           int64_t* activation_bytes);
int ace355_vae_hop(const ace355_vae* h);
/* Encoder half (vae_model.py:92-116, 148-187, 285-310): available when the encoder.* keys of
 * AutoencoderOobleck.state_dict() were loaded before ace355_vae_finalize.  audio dev f32 [B, audio_channels, L];
 * latents_out dev f32 [B, 64, T] with T = ace355_vae_latent_frames(h, L) (= L / hop for multiples of the hop);
 * noise dev f32 [B, 64, T] -> `latent_dist.sample()` = mean + (softplus(scale) + 1e-4) * noise
 * (handler/vae_encode.py:66); noise NULL -> the mean (`latent_dist.mode()`). */
int ace355_vae_encode(ace355_vae* h, const float* audio_dev, const float* noise_dev, int B, int64_t L, float* latents_out_dev,
                      void* stream);
int ace355_vae_latent_frames(const ace355_vae* h, int64_t L);
int ace355_vae_set_profile(ace355_vae* h, int enable);
int ace355_vae_get_profile(ace355_vae* h, double* conv_ms, double* conv_flops, int64_t* conv_launches);

/* Test / debug hooks: the stored activations of a decode or an encode, one STAGE per stored tensor, in launch order.
 * Decoder: the bf16 NLC image of z; conv1; per block the transposed conv and its three residual units (the waveform is the call's own
 * output).  Encoder: the im2col image of the audio; the first conv; per block the three units and the strided conv; the head (mean | scale,
 * before the Gaussian arithmetic).  A residual unit that runs as ONE launch is one stage (UNIT); one that runs as two launches is two
 * (UNIT_K7: the k = 7 result as stored for the k = 1 conv, UNIT_K1: the unit's output), so every stage but INPUT is the output of exactly
 * one conv launch.  Which form a unit takes, and where the Snakes are applied, depends on the width and on the A/B switches of the process
 * (ACE355_CONV_FUSE_RU, ACE355_VAE_EPISNAKE): the flags below say it, so a test never hard-codes the rounding points.
 * The list is not written down anywhere: it is read off the steps of plan_vae (csrc/vae_plan.h; ace355_vae_plan below), the same steps
 * the decode and the encode execute, so a stage and its launch cannot disagree. */
#define ACE355_VAE_STAGE_INPUT 0   /* decoder: bf16(z) as [T][64]; encoder: bf16 im2col rows [L][64], column k * audio_channels + c = audio[c][l + k - 3] */
#define ACE355_VAE_STAGE_CONV_IN 1 /* decoder.conv1 / encoder.conv1 */
#define ACE355_VAE_STAGE_CONVT 2   /* decoder.block.{block}.conv_t1 */
#define ACE355_VAE_STAGE_UNIT 3    /* ...block.{block}.res_unit{unit + 1}, one launch */
#define ACE355_VAE_STAGE_UNIT_K7 4 /* ...res_unit{unit + 1}.conv1 (+ snake2 when OUT_SNAKE) */
#define ACE355_VAE_STAGE_UNIT_K1 5 /* ...res_unit{unit + 1}.conv2 + the unit's input */
#define ACE355_VAE_STAGE_DOWN 6    /* encoder.block.{block}.conv1 (strided) */
#define ACE355_VAE_STAGE_HEAD 7    /* encoder.conv2: f32 [2 * latent channels][T] per item */
#define ACE355_VAE_FLAG_IN_SNAKE 1  /* the launch applies the layer's input Snake while staging its input (rounded to bf16 there) */
#define ACE355_VAE_FLAG_OUT_SNAKE 2 /* the stored tensor already carries its (single) reader's Snake, applied to the fp32 sum */
#define ACE355_VAE_FLAG_FUSED 4     /* residual unit in one launch: the k = 7 result meets snake2 unrounded and is never stored */
#define ACE355_VAE_FLAG_F32_NCL 8   /* stored as f32 [channels][rows] per item; otherwise bf16 [rows][channels] */
typedef struct ace355_vae_stage_info {
    int32_t kind;      /* ACE355_VAE_STAGE_* */
    int32_t block;     /* block index, -1 outside the blocks */
    int32_t unit;      /* residual unit 0..2, -1 otherwise */
    int32_t channels;
    int32_t flags;     /* ACE355_VAE_FLAG_* */
    int32_t src;       /* stage the launch reads (-1: the call's input) */
    int32_t res;       /* stage added as the residual, -1: none */
    int32_t dilation;  /* of the k = 7 conv of a unit, else 1 */
    int64_t rows;      /* per item */
} ace355_vae_stage_info;
/* Number of stages of the decoder (encoder == 0) or the encoder; negative before finalize / without encoder weights. */
int ace355_vae_num_stages(const ace355_vae* h, int encoder);
/* Stage `stage` of a decode of T latent frames (encoder == 0) or an encode of T audio samples per item. */
int ace355_vae_get_stage(const ace355_vae* h, int encoder, int stage, int64_t T, ace355_vae_stage_info* out);
/* After stage `stage` of every following decode / encode, copy the stored activation of the whole batch ([B] x the stage's per-item
 * layout) to dst_dev (hipMemcpyAsync on the call's stream); capacity_bytes is checked against the stage's size at each call
 * (ACE355_ERR_INVALID).  dst_dev NULL clears the tap; several stages may be tapped at once.  A tapped call must run as ONE whole-sequence
 * window over the whole batch: if the budget splits it, it returns ACE355_ERR_STATE and launches nothing.  Taps only observe: the conv
 * launches and their arguments are those of an untapped call. */
int ace355_vae_set_tap(ace355_vae* h, int encoder, int stage, void* dst_dev, int64_t capacity_bytes);

/* The conv launches of one decode window or one encode group as data, in launch order: plan_vae of csrc/vae_plan.h, which
 * ace355_vae_decode / _encode execute step by step.  A step names everything its launch takes except pointers.  No GPU, no handle. */
#define ACE355_VAE_W_CONV_IN 0  /* decoder.conv1 / encoder.conv1 */
#define ACE355_VAE_W_CONVT 1    /* decoder.block.{block}.conv_t1 */
#define ACE355_VAE_W_UNIT_C1 2  /* ...block.{block}.res_unit{unit + 1}.conv1 (fused: + conv2 and snake2 inside the launch) */
#define ACE355_VAE_W_UNIT_C2 3  /* ...res_unit{unit + 1}.conv2 */
#define ACE355_VAE_W_DOWN 4     /* encoder.block.{block}.conv1 */
#define ACE355_VAE_W_OUT 5      /* decoder.conv2 */
#define ACE355_VAE_W_HEAD 6     /* encoder.conv2 */
#define ACE355_VAE_SNAKE_NONE 0
#define ACE355_VAE_SNAKE_UNIT_S1 1 /* block.{snake_block}.res_unit{unit + 1}.snake1 */
#define ACE355_VAE_SNAKE_UNIT_S2 2 /* ...snake2 */
#define ACE355_VAE_SNAKE_BLOCK 3   /* block.{snake_block}.snake1 */
#define ACE355_VAE_SNAKE_FINAL 4   /* decoder.snake1 / encoder.snake1 */
#define ACE355_VAE_BUF_NONE (-1)
#define ACE355_VAE_BUF_SLOT0 0     /* 0 .. 2: the three ping-pong activation buffers */
#define ACE355_VAE_BUF_IN 3        /* the call's input image (bf16 latent rows / im2col'ed audio rows) */
#define ACE355_VAE_BUF_OUT 4       /* the call's output (the waveform / the encoder head's f32 image) */
typedef struct ace355_vae_step_info {
    int32_t weight, block, unit;                   /* ACE355_VAE_W_* and where; -1 outside the blocks / units */
    int32_t fused;
    int32_t in_snake, in_snake_block;              /* ACE355_VAE_SNAKE_*: applied while staging the input */
    int32_t out_snake, out_snake_block;            /* the single reader's Snake, applied by this launch's epilogue */
    int32_t src, dst, res;                         /* ACE355_VAE_BUF_* */
    int32_t Cin, N, taps, dil, center, L_in, M;    /* as ConvArgs (csrc/common.h) */
    int32_t out_mode, n_real, ncl_m_lo, ncl_m_hi;
    int32_t stage;                                 /* index of the public stage this launch stores, -1: none (the decoder's output conv) */
    int32_t reserved;
    int64_t src_off;                               /* elements from the start of the source buffer's first item (a decode window's first row) */
    int64_t x_batch_stride, x_shift, x_valid, res_batch_stride, y_batch_stride, y_shift, y_valid, ncl_ld, ncl_off;
    ace355_vae_stage_info stage_info;              /* valid when stage >= 0 */
    ace355_conv_plan_info plan;
} ace355_vae_step_info;
typedef struct ace355_vae_plan_info {
    int32_t items_per_window, core_frames, overlap_frames;   /* decoder: the window plan; encoder: items per group, 0, 0 */
    int32_t n_steps, n_stages;
    int32_t reserved;
    int64_t window_len;        /* latent frames (decoder) / samples (encoder) per item the steps cover */
    int64_t out_len;           /* per item: samples the window decodes / latent frames */
    int64_t slot_elems;        /* bf16 elements per item of each ping-pong buffer: the largest extent a step writes */
    int64_t activation_bytes;  /* of the buffers the budget counts, for items_per_window items */
} ace355_vae_plan_info;
/* The steps of the FIRST window of a decode of (B, T latent frames) or the first group of an encode of (B, T samples) under a budget in
 * bytes (0: the default of a new handle) and, for the decoder, a window overlap in frames (0: the default).  steps_out may be NULL or
 * shorter than the plan (capacity): n_out is the plan's step count either way. */
int ace355_vae_plan(const ace355_vae_config* cfg, int encoder, int B, int64_t T, int64_t budget_bytes, int overlap_frames,
                    ace355_vae_step_info* steps_out, int capacity, int32_t* n_out, ace355_vae_plan_info* info_out);

/* ------------------------------------------------------------------------------------------
 * Condition encoder: AceStepConditionEncoder.forward, base.py:1509-1554
 * = text_projector + AceStepLyricEncoder (base.py:577-731) + AceStepTimbreEncoder (base.py:997-1178)
 * + pack_sequences x2 (base.py:138-169).  Replaces the call `self.encoder(...)` of prepare_condition
 * (base.py:1626-1633); its output is what ace355_dit_set_condition takes.
 * ---------------------------------------------------------------------------------------- */
typedef struct ace355_cond ace355_cond;

typedef struct ace355_cond_config {
    int32_t hidden_size;        /* 2048 */
    int32_t intermediate_size;  /* 6144 */
    int32_t num_heads;          /* 16 */
    int32_t num_kv_heads;       /* 8 */
    int32_t head_dim;           /* 128 (only value supported) */
    int32_t text_hidden_dim;    /* 1024: text and lyric embedding width */
    int32_t timbre_hidden_dim;  /* 64: reference-audio latent width */
    int32_t num_lyric_layers;   /* 8 */
    int32_t num_timbre_layers;  /* 4 */
    int32_t sliding_window;     /* 128 */
    uint64_t sliding_layer_mask; /* bit i set: encoder layer i is "sliding_attention" (config.layer_types[i]) */
    float rms_norm_eps;         /* 1e-6 */
    float rope_theta;           /* 1e6 */
} ace355_cond_config;

int ace355_cond_create(const ace355_cond_config* cfg, ace355_cond** out);
void ace355_cond_destroy(ace355_cond* h);
/* name = a key of AceStepConditionEncoder.state_dict() (`model.encoder` of the reference checkpoint), e.g.
 * "lyric_encoder.layers.3.self_attn.q_proj.weight"; "timbre_encoder.special_token" is accepted and ignored
 * (the reference's forward never reads it).  Same contract as ace355_dit_load_tensor. */
int ace355_cond_load_tensor(ace355_cond* h, const char* name, const void* data, int dtype, int64_t numel, int is_device);
int ace355_cond_finalize(ace355_cond* h);
/* Rows per item of the packed output: Ll + (max number of reference clips of one item) + Lt; < 0 on bad arguments. */
int ace355_cond_out_len(int Ll, int Lt, const int32_t* refer_item_host, int Nref, int B);
/* One encoder forward.  text dev f32 [B,Lt,text_dim], lyric dev f32 [B,Ll,text_dim], refer dev f32
 * [Nref,Tref,timbre_dim] (refer_audio_acoustic_hidden_states_packed); text_len / lyric_len host int32 [B]: the
 * attention masks in prefix form (mask[b][j] = j < len[b]; anything else must take the PyTorch path);
 * refer_item host int32 [Nref] = refer_audio_order_mask.  Writes enc_out dev f32 [B, out_len, hidden]
 * (encoder_hidden_states, valid tokens first exactly as pack_sequences orders them, padding rows included because the
 * DiT attends them: base.py:1384-1385) and enc_len_out host int32 [B] (encoder_attention_mask in prefix form). */
int ace355_cond_encode(ace355_cond* h, const float* text_dev, const int32_t* text_len_host, int Lt, const float* lyric_dev,
                       const int32_t* lyric_len_host, int Ll, const float* refer_dev, const int32_t* refer_item_host,
                       int Nref, int Tref, int B, float* enc_out_dev, int32_t* enc_len_out_host, void* stream);

/* ------------------------------------------------------------------------------------------
 * Caption text encoder: transformers' Qwen3Model as the reference loads it (Qwen3-Embedding-0.6B,
 * init_service_loader.py:146-161) = embed_tokens + num_layers pre-norm decoder layers with causal GQA self-attention + final
 * RMSNorm.  Replaces `self.text_encoder(input_ids=..., lyric_attention_mask=None).last_hidden_state` and
 * `self.text_encoder.embed_tokens(ids)` of conditioning_embed.py:71-79.  No attention mask: right-padded ids run purely causally.
 * ---------------------------------------------------------------------------------------- */
typedef struct ace355_textenc ace355_textenc;

#define ACE355_TEXTENC_MAX_TOKENS 65536 /* ids per encode / embed call (the reference sends at most 16 x 256 or 8 x 2048) */

typedef struct ace355_textenc_config {
    int32_t hidden_size;        /* 1024 */
    int32_t intermediate_size;  /* 3072 */
    int32_t num_layers;         /* 28 */
    int32_t num_heads;          /* 16: must be 2 * num_kv_heads */
    int32_t num_kv_heads;       /* 8 */
    int32_t head_dim;           /* 128 (only value supported) */
    int32_t vocab_size;         /* 151669 */
    float rms_norm_eps;         /* 1e-6 */
    float rope_theta;           /* 1e6 */
} ace355_textenc_config;

/* ACE355_ERR_UNSUPPORTED for head_dim != 128 or num_heads != 2 * num_kv_heads. */
int ace355_textenc_create(const ace355_textenc_config* cfg, ace355_textenc** out);
void ace355_textenc_destroy(ace355_textenc* h);
/* name = a key of Qwen3Model.state_dict() ("embed_tokens.weight", "layers.3.self_attn.q_proj.weight", "norm.weight", ...);
 * the rotary buffers are not tensors of this call.  Same contract as ace355_dit_load_tensor. */
int ace355_textenc_load_tensor(ace355_textenc* h, const char* name, const void* data, int dtype, int64_t numel, int is_device);
int ace355_textenc_finalize(ace355_textenc* h);
/* ids host int32 [N, S] -> out dev bf16 [N, S, hidden] (last_hidden_state).  Ids outside [0, vocab) are refused with
 * ACE355_ERR_INVALID before anything is launched.  The ids are copied before the call returns. */
int ace355_textenc_encode(ace355_textenc* h, const int32_t* ids_host, int N, int S, void* out_dev, void* stream);
/* ids host int32 [n] -> out dev bf16 [n, hidden] = rows of embed_tokens.weight (out 16-byte aligned); same id check. */
int ace355_textenc_embed(ace355_textenc* h, const int32_t* ids_host, int64_t n, void* out_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * 5 Hz LM forward: transformers' Qwen3ForCausalLM (0.6B / 1.7B) as LLMHandler._forward_pass calls it
 * (llm_inference.py:416-438) = the text encoder's stack + a KV cache + the LM head, for left-padded batches of N <= 16 sequences
 * that advance one token per step.  Only the forward: the caller samples from the returned last-position logits.
 *
 * Positions are padded column indices (no position_ids are passed, so pads are not subtracted): the token in column j has RoPE
 * position j, and the query in column i of sequence n sees keys first[n] <= j <= i, first[n] = number of leading pad columns.
 * Pad columns' K / V are stored and never visible; their outputs are zeros or finite and never read.
 * Cache: bf16 [layer][K|V][max_seqs][kv head][max_positions][128], allocated at the first prefill, kept for the handle's life.
 * ---------------------------------------------------------------------------------------- */
typedef struct ace355_lm ace355_lm;

#define ACE355_LM_MAX_SEQS 16         /* lm_batch_chunk_size 8, doubled by CFG */
#define ACE355_LM_MAX_POSITIONS 16384 /* largest max_positions */
#define ACE355_LM_MAX_TOKENS 65536    /* N * P of one prefill */

typedef struct ace355_lm_config {
    int32_t hidden_size;        /* 1024 (0.6B), 2048 (1.7B) */
    int32_t intermediate_size;  /* 3072, 6144 */
    int32_t num_layers;         /* 28 */
    int32_t num_heads;          /* 16: must be 2 * num_kv_heads */
    int32_t num_kv_heads;       /* 8 */
    int32_t head_dim;           /* 128 (only value supported) */
    int32_t vocab_size;         /* Qwen3's vocabulary plus the audio-code tokens: whatever the checkpoint says */
    float rms_norm_eps;         /* 1e-6 */
    float rope_theta;           /* 1e6 */
    int32_t tie_word_embeddings; /* 1: the head reads embed_tokens.weight; "lm_head.weight" is accepted and dropped */
    int32_t max_seqs;           /* 1 .. ACE355_LM_MAX_SEQS */
    int32_t max_positions;      /* 1 .. ACE355_LM_MAX_POSITIONS: prompt + generated tokens */
} ace355_lm_config;

/* ACE355_ERR_UNSUPPORTED for head_dim != 128 or num_heads != 2 * num_kv_heads (Qwen3-4B, 32 / 8 heads, needs ace355_lm_create_ex).
 * The same as ace355_lm_create_ex(cfg, 0, out). */
int ace355_lm_create(const ace355_lm_config* cfg, ace355_lm** out);
/* The config struct is frozen, so what a caller opts into travels beside it.  ACE355_LM_ALLOW_GQA4: num_heads == 4 * num_kv_heads is
 * accepted next to 2 * (Qwen3-4B: hidden 2560, intermediate 9728, 36 layers, 32 / 8 heads of 128).  Every call on such a handle is
 * the one documented below; the 2 : 1 kernels' operations and their order are unchanged.  ACE355_ERR_UNSUPPORTED for every other
 * ratio and for head_dim != 128, ACE355_ERR_INVALID for an unknown flag bit. */
#define ACE355_LM_ALLOW_GQA4 1u
int ace355_lm_create_ex(const ace355_lm_config* cfg, uint32_t flags, ace355_lm** out);
void ace355_lm_destroy(ace355_lm* h);
/* name = a key of Qwen3ForCausalLM.state_dict(): "model.embed_tokens.weight", "model.layers.<i>.*", "model.norm.weight",
 * "lm_head.weight".  Same contract as ace355_dit_load_tensor. */
int ace355_lm_load_tensor(ace355_lm* h, const char* name, const void* data, int dtype, int64_t numel, int is_device);
int ace355_lm_finalize(ace355_lm* h);
/* Step 0: resets the cache, runs ids host int32 [N, P] (first host int32 [N]: leading pad columns per sequence), stores every
 * layer's K / V, leaves the length at P and writes the logits of column P - 1: logits dev f32 [N, vocab].  ACE355_ERR_INVALID
 * before anything is launched, with the handle unchanged, for ids outside [0, vocab), first[n] outside [0, P), N > max_seqs,
 * P > max_positions, N * P > ACE355_LM_MAX_TOKENS.  ids and first are copied before the call returns. */
int ace355_lm_prefill(ace355_lm* h, const int32_t* ids_host, const int32_t* first_host, int N, int P, float* logits_dev, void* stream);
/* Step t > 0: one more position for all N sequences of the prefill, ids host int32 [N]; logits dev f32 [N, vocab].  Refused like
 * prefill for bad ids, without a prefill and at length == max_positions. */
int ace355_lm_decode(ace355_lm* h, const int32_t* ids_host, float* logits_dev, void* stream);
/* Positions held by the cache (0 before the first prefill); < 0 for a null handle. */
int ace355_lm_length(ace355_lm* h);
/* The decode attention's cut of a cache of `length` keys (csrc/lm_plan.h): keys per workgroup and chunks per sequence.  A pure
 * function of the length alone - no GPU, no handle. */
int ace355_lm_decode_plan(int length, int32_t* chunk_out, int32_t* splits_out);

/* Teacher-forced scoring (csrc/lm_score.hip; the reference's acestep/core/scoring/lm_score.py needs, per target token, one
 * log-probability and one rank - not the [T, V] logits it copies to the host).
 *
 * ace355_lm_score_rows is handle-free: R rows of bf16 activations against a bf16 head W [V, D] (row stride D), one target id per row.
 *   row r          = x[row_index[r] * x_row_stride ..] (x[r * x_row_stride ..] when row_index_dev is NULL)
 *   logit[r][v]    = sum_k row_r[k] * W[v][k], fp32 accumulation on the matrix cores
 *   logprob_out[r] = logit[r][t_r] - logsumexp_v logit[r][v], clamped to <= 0               (fp32 [R])
 *   rank_out[r]    = #{v != t_r : logit[r][v] > z_r, or logit[r][v] == z_r and v < t_r}     (int32 [R], 0 = the target is the argmax)
 * with z_r the target's own logit: equal values are ordered by ascending id, as ace355_lm_pick orders them.  Three launches on
 * `stream`, no atomics: the same call gives the same bits, and a row's bits do not depend on R or on the other rows.  No logits are
 * stored; ids >= V are masked and no row of W at or beyond V is read, so V needs no padding.  row_index and targets are device
 * memory and are NOT checked: row_index must name rows of x; a target outside [0, V) yields log-prob NaN and rank -1.
 * ACE355_ERR_INVALID before any HIP call for R outside 1 .. ACE355_LM_MAX_TOKENS, V outside 1 .. 1 << 20, D no multiple of 64 or
 * above 16384, x_row_stride < D or no multiple of 8, a null pointer other than row_index_dev, x / W / workspace not 16-byte
 * aligned, or a workspace smaller than ace355_lm_score_workspace_bytes(R, V). */
int ace355_lm_score_rows(const void* x_dev, int64_t x_row_stride, const int32_t* row_index_dev, const void* W_dev,
                         const int32_t* targets_dev, int R, int V, int D, float* logprob_out, int32_t* rank_out, void* workspace_dev,
                         size_t workspace_bytes, void* stream);
/* Bytes of workspace ace355_lm_score_rows needs: the thresholds and one 32-byte partial per (row, chunk).  Pure; 0 for R or V outside
 * the limits above. */
size_t ace355_lm_score_workspace_bytes(int R, int V);
/* What ace355_lm_score_rows launches (csrc/lm_plan.h: plan_lm_score): rows per workgroup, ids per workgroup (a function of V alone),
 * chunks = ceil(V / chunk), and the fused head's grid (x = row tiles, y = chunks).  Chunk c holds ids [c * chunk, min(V, (c + 1) *
 * chunk)).  Pure: no GPU, no handle.  ACE355_ERR_INVALID for a request ace355_lm_score_rows would refuse for its sizes. */
int ace355_lm_score_plan(int R, int V, int D, int32_t* tile_rows_out, int32_t* chunk_out, int32_t* chunks_out, int32_t* grid_x_out,
                         int32_t* grid_y_out);
/* Scores the columns [start[n], P) of every sequence of a left-padded batch (ids, first, N, P as for ace355_lm_prefill; start host
 * int32 [N], first[n] < start[n] < P): the same upload, embedding and stack as a prefill, then ace355_lm_score_rows on the final
 * norm of the rows that predict those columns (row n * P + c - 1 predicts ids[n][c]) and the handle's head.  Outputs are compact, in
 * (n, c) order: logprob dev f32 [R], rank dev int32 [R], R = sum_n (P - start[n]).  Refused like ace355_lm_prefill, and for a start
 * outside (first, P), before anything is launched and with the handle unchanged.  Afterwards the handle holds NO generation
 * (ace355_lm_length is 0; a decode is refused): scoring is not a prefill.  The scoring workspace belongs to the handle and grows on
 * demand.  ids, first and start are copied before the call returns. */
int ace355_lm_score(ace355_lm* h, const int32_t* ids_host, const int32_t* first_host, const int32_t* start_host, int N, int P,
                    float* logprob_dev, int32_t* rank_dev, void* stream);

/* One pass of the encoder stack behind ace355_cond (two stacks), ace355_detok, ace355_tok, ace355_textenc and ace355_lm as data, in
 * launch order: plan_encoder_pass of csrc/encoder_plan.h, which those handles execute step by step.  One step is one call of a launcher
 * with everything it takes except pointers; buffers appear as roles.  No GPU, no handle. */
#define ACE355_ENC_STEP_RMSNORM 0       /* launch_rmsnorm_mod: h -> xn (norm 0: input_layernorm, 1: post_attention_layernorm), h -> out (2: the final norm) */
#define ACE355_ENC_STEP_GEMM 1          /* launch_gemm */
#define ACE355_ENC_STEP_KV_STORE 2      /* launch_kv_store: the K / V columns of the QKV rows -> the cache at positions pos0 .. pos0 + Sq - 1 */
#define ACE355_ENC_STEP_CAUSAL_ATTN 3   /* launch_causal_attention over the QKV rows */
#define ACE355_ENC_STEP_DECODE_ATTN 4   /* launch_decode_attention over `len` keys of the cache */
#define ACE355_ENC_STEP_TRANSPOSE_V 5   /* launch_transpose_v */
#define ACE355_ENC_STEP_VMEAN 6         /* launch_vmean */
#define ACE355_ENC_STEP_ATTN 7          /* launch_attention (bidirectional) */
#define ACE355_ENC_STEP_KINDS 8
#define ACE355_ENC_PROJ_QKV 0
#define ACE355_ENC_PROJ_O 1
#define ACE355_ENC_PROJ_GATE_UP 2
#define ACE355_ENC_PROJ_DOWN 3
#define ACE355_ENC_BUF_NONE (-1)
#define ACE355_ENC_BUF_H 0              /* residual stream f32 [M][D]: the pass's input, embedded by the caller */
#define ACE355_ENC_BUF_XN 1             /* normed rows bf16 [M][D] */
#define ACE355_ENC_BUF_QKV 2            /* q | k | v rows bf16 [M + 64][QKV] */
#define ACE355_ENC_BUF_AO 3             /* attention output bf16 [M][QD] */
#define ACE355_ENC_BUF_ACT 4            /* SwiGLU output bf16 [M][F] */
#define ACE355_ENC_BUF_VT 5             /* V^T bf16 [N][KVH][128][Sp] */
#define ACE355_ENC_BUF_VMEAN 6          /* mean V row bf16 [N][KVH][128] */
#define ACE355_ENC_BUF_CACHE 7          /* the handle's KV cache */
#define ACE355_ENC_BUF_OUT 8            /* the call's output bf16 [M][D] */
typedef struct ace355_encoder_pass_request {
    int32_t hidden_size, intermediate_size, num_heads, num_kv_heads, num_layers;
    int32_t sliding_window;
    int32_t causal;                          /* 1: the text encoder's and the LM's stack; 0: bidirectional */
    int32_t N, S;                            /* sequences, rows per sequence */
    int32_t has_kv_len;                      /* a per-sequence key count is given (bidirectional only) */
    int32_t has_cache;                       /* a KV cache is given (causal only), with ... */
    int32_t pos0, max_pos, max_seqs;         /* ... the position of the call's first row, and the cache's capacity */
    int32_t has_first;                       /* ... and per-sequence first visible keys (left padding) */
    int32_t reserved;
    uint64_t sliding_layer_mask;             /* bit l: layer l is sliding (bidirectional only; a causal stack does not read it) */
} ace355_encoder_pass_request;
typedef struct ace355_encoder_step_info {
    int32_t kind, layer;                     /* ACE355_ENC_STEP_*; layer -1: the final norm */
    int32_t src, dst;                        /* ACE355_ENC_BUF_*: the row operand read, the buffer written */
    int32_t M, N, K;                         /* GEMM sizes; a norm: M rows of N columns */
    int32_t norm;                            /* rmsnorm: which weight (see ACE355_ENC_STEP_RMSNORM); -1 otherwise */
    int32_t proj;                            /* GEMM: ACE355_ENC_PROJ_*; -1 otherwise */
    int32_t lda, ldw, ldc, mode;             /* GEMM: leading dimensions and GemmEpilogue::mode */
    int32_t rows_per_seq;                    /* norms and GEMMs */
    int32_t hn_q_cols, hn_qk_cols;           /* mode 4: the head-norm columns */
    int32_t rope_row0;                       /* mode 4: row of the rope tables that row 0 of every sequence takes (= pos0) */
    int32_t sk_cnt;                          /* mode 2: the handle's split-K counters are bound */
    /* kv_store, the attentions, transpose_v, vmean */
    int32_t seqs, Sq, Skv;
    int32_t Hq, Hkv;
    int32_t ld, k_col0, v_col0, o_ld;        /* row stride of the QKV rows, first K / V column, row stride of the output */
    int32_t Sp;                              /* transpose_v, attention: the V^T row pitch */
    int32_t window;                          /* attention: the layer's window, -1: none */
    int32_t kv_len, first;                   /* attention: key counts (and vmean) bound; causal: first visible keys bound */
    int32_t pos0;                            /* kv_store */
    int32_t len, chunk, splits;              /* decode attention: keys, and plan_lm_decode(len) */
    int32_t reserved;
    double flops;                            /* GEMM: 2 M N K */
} ace355_encoder_step_info;
typedef struct ace355_encoder_pass_info {
    int32_t M, Sp, QKV;                      /* rows, padded V^T pitch, QKV width */
    int32_t rope_rows;                       /* rows of the rope tables the pass needs */
    int32_t n_steps;
    int32_t calls[ACE355_ENC_STEP_KINDS];    /* launcher calls per kind */
    int32_t reserved;
    double gemm_flops;
} ace355_encoder_pass_info;
/* A refusal is ACE355_ERR_INVALID with the text the stack or its launchers give.  steps_out may be NULL or shorter than the plan. */
int ace355_encoder_pass_plan(const ace355_encoder_pass_request* request, ace355_encoder_step_info* steps_out, int capacity,
                             int32_t* n_out, ace355_encoder_pass_info* info_out);

/* ------------------------------------------------------------------------------------------
 * 5 Hz LM token selection: top-k, top-p and the draw on logits that already exist, i.e. what
 * LLMHandler._apply_top_k_filter, _apply_top_p_filter and _sample_tokens (llm_inference.py:367-399) do in that order.  No handle,
 * no state; the logits are only read.
 *
 * A row is V fp32 logits, each finite or -inf (-0.0 == +0.0).  A row with a NaN, a +inf or no finite entry yields token -1, kept
 * count 0 and an all-zero mask.
 *   top-k (0 < top_k < V): t = the k-th largest value counted with multiplicity; x survives iff x >= t (t == -inf removes nothing).
 *   top-p (0 < top_p < 1), over the survivors: m_i = exp(x_i - max), Z = sum; walk in descending value, equal values in ascending id;
 *     position 0 is kept, position j >= 1 iff the mass of positions 0 .. j-1 is <= top_p * Z.
 *   kept = finite and survives both.
 *   temperature <= 0: the largest kept logit, lowest id on a tie.  temperature T > 0: w_i = exp((x_i - max) / T) over the kept
 *     entries, total W; in ascending id with running sum S the token is the first kept id with S > u * W, else the last kept id with
 *     a non-zero weight: inverse-CDF sampling of softmax(filtered / T) with the caller's u in [0, 1).
 * Exponentials and sums are fp64, summed in an order that depends on V alone; a row's results do not depend on B, on the other rows
 * or on the run.
 * ---------------------------------------------------------------------------------------- */
typedef struct ace355_lm_pick_params { int32_t top_k; float top_p; float temperature; int32_t reserved; } ace355_lm_pick_params;
/* Bytes of workspace ace355_lm_pick needs for B rows of V logits.  Pure; 0 for B outside 1 .. ACE355_LM_MAX_SEQS or V outside
 * 1 .. 1 << 20. */
size_t ace355_lm_pick_workspace_bytes(int B, int V);
/* The cut of a row over workgroups (csrc/lm_plan.h): ids per chunk and chunks per row.  A pure function of V alone - no GPU. */
int ace355_lm_pick_plan(int V, int32_t* chunk_out, int32_t* chunks_out);
/* logits dev f32, row b at logits + b * row_stride; u dev f32 [B] (may be NULL when temperature <= 0); tokens dev int64 [B];
 * kept dev int32 [B] or NULL; keep dev uint8 [B, V] or NULL; workspace dev, 8-byte aligned.  ACE355_ERR_INVALID before any HIP call
 * for B outside 1 .. ACE355_LM_MAX_SEQS, V outside 1 .. 1 << 20, row_stride < V, a null required pointer, u == NULL with
 * temperature > 0, or a workspace smaller than ace355_lm_pick_workspace_bytes(B, V). */
int ace355_lm_pick(const float* logits_dev, int64_t row_stride, int B, int V, const ace355_lm_pick_params* p, const float* u_dev,
                   int64_t* tokens_dev, int32_t* kept_dev, uint8_t* keep_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * 5 Hz LM logits stage: what the reference's CFG loop does to the logits between its forward and its
 * token selection (llm_inference.py:2482-2493): the CFG combine, the CODES_GENERATION / COMPLETED / disabled branches of
 * MetadataConstrainedLogitsProcessor.__call__ with _apply_temperature_scaling, then transformers' RepetitionPenaltyLogitsProcessor.
 * No handle, no state, one launch.
 *
 * For every row b and id v, in this order, every operation rounded to fp32 on its own (never contracted into an fma):
 *   1. x = u + cfg_scale * (c - u) with c = cond[b][v], u = uncond[b][v]; x = c when uncond is NULL.
 *   2. x = x + mask[v] when mask is given (a real add: -0.0 + 0.0 is +0.0, NaN propagates).
 *   3. eos_mode 1 (block): x = -inf at v == eos_id.  eos_mode 2 (force): x = -inf at every v != eos_id; eos_id keeps step 2's value.
 *   4. x = x / temperature when has_temperature (IEEE division, correctly rounded).  The caller maps the reference's T <= 0 to 1e-6.
 *   5. when penalty != 1 and bit v & 31 of seen[b][v >> 5] is set: x = x < 0 ? x * penalty : x / penalty.
 *   out[b][v] = x.
 * ---------------------------------------------------------------------------------------- */
typedef struct ace355_lm_shape_params {
    float cfg_scale;         /* read only when uncond is given */
    int32_t eos_id;          /* read only when eos_mode != 0 */
    int32_t eos_mode;        /* 0 none, 1 block, 2 force */
    int32_t has_temperature; /* 0: step 4 is skipped */
    float temperature;       /* > 0 when has_temperature */
    float penalty;           /* finite, > 0; 1 = off */
    const float* mask;       /* dev f32 [V], or NULL */
    const uint32_t* seen;    /* dev u32 [B, (V + 31) / 32], rows dense; NULL iff penalty == 1 */
} ace355_lm_shape_params;
/* cond, uncond (or NULL), out: dev f32, row b at base + b * stride, each stride >= V, rows only 4-byte aligned; out may be cond
 * (an element is read before it is written, by the same thread) and must not overlap anything else.  ACE355_ERR_INVALID before any
 * HIP call for B outside 1 .. ACE355_LM_MAX_SEQS, V outside 1 .. 1 << 20, a stride < V, a null cond / out / params, eos_mode outside
 * 0 .. 2, eos_mode != 0 with eos_id outside [0, V), a penalty that is not finite or <= 0, seen == NULL with penalty != 1, a NaN
 * cfg_scale with uncond given, has_temperature with temperature <= 0 or NaN. */
int ace355_lm_shape(const float* cond_dev, int64_t cond_stride, const float* uncond_dev, int64_t uncond_stride, float* out_dev,
                    int64_t out_stride, int B, int V, const ace355_lm_shape_params* p, void* stream);
/* The stage in the model's dtype: what the reference's non-CFG loop (_generate_with_constrained_decoding,
 * llm_inference.py:2369-2377) does to outputs.logits[:, -1, :], which it never upcasts, so that on a bf16 model each of the
 * processor's torch kernels rounds its result to bf16.  The arguments of ace355_lm_shape plus `dtype`; one launch of the same grid.
 *   ACE355_DTYPE_F32: exactly ace355_lm_shape.
 *   ACE355_DTYPE_BF16: r(x) is round-to-nearest-even of an fp32 value to bf16, kept in fp32 (NaN stays NaN, +-inf and +-0 stay,
 *     subnormals round like any value, a finite value beyond bf16's largest becomes inf).  For every row b and id v:
 *       1. x = r(cond[b][v]) (the reference's cast of the logits to the model's dtype); x = r(x + r(mask[v])) when mask is given.
 *       2. the EOS rule of ace355_lm_shape's step 3, unchanged.
 *       3. x = r(x / temperature) when has_temperature: the IEEE fp32 division by the fp32 temperature, then r.
 *       4. on seen ids x = x < 0 ? r(x * penalty) : r(x / penalty), in fp32 by the fp32 penalty, then r.
 *     out stays fp32 and holds bf16-representable values.  The rounding is an integer operation on the bit pattern.
 *   This is torch on the CPU, bit for bit: there `x / T` on a bf16 tensor is r(fp32(x) / fp32(T)), and `x * p`, `x / p` likewise.
 *   torch on the GPU may turn the division by a host scalar into a multiplication by its reciprocal; the stage keeps the IEEE
 *   division of the fp32 stage and of torch on the CPU, so that one oracle serves both.  At T = 0.6 the two readings differ in
 *   about 1 % of the bf16 results; which of them a GPU reference run produces is not pinned.
 * ACE355_ERR_INVALID before any HIP call for a dtype other than the two, for uncond != NULL with a dtype other than
 * ACE355_DTYPE_F32 (the reference never combines below fp32), and for everything ace355_lm_shape refuses. */
int ace355_lm_shape_as(const float* cond_dev, int64_t cond_stride, const float* uncond_dev, int64_t uncond_stride, float* out_dev,
                       int64_t out_stride, int B, int V, const ace355_lm_shape_params* p, int dtype, void* stream);
/* ids dev int64, row b at ids + b * row_stride, T ids per row: sets bit v & 31 of seen[b][v >> 5] for every id v in [0, V) with an
 * integer atomic OR (commutative: the result does not depend on order); ids outside [0, V) are ignored.  Bits are only ever set:
 * the caller zeroes the bitmap (dev u32 [B, (V + 31) / 32]).  ACE355_ERR_INVALID before any HIP call for B outside
 * 1 .. ACE355_LM_MAX_SEQS, V outside 1 .. 1 << 20, T outside 1 .. ACE355_LM_MAX_POSITIONS, row_stride < T, a null pointer. */
int ace355_lm_seen_mark(const int64_t* ids_dev, int64_t row_stride, int B, int T, int V, uint32_t* seen_dev, void* stream);
/* ace355_lm_decode with ids that never visit the host: tokens dev int64 [B], n_seqs % B == 0, sequence n takes tokens[n % B] (the
 * reference's next_tokens.repeat(2, 1)).  One small kernel writes the handle's id buffer, the rest is ace355_lm_decode's; the call
 * makes no stream synchronisation.  A token outside [0, vocab) cannot be refused on the host: id 0 is embedded in its place and a
 * device counter is bumped (ace355_lm_bad_tokens).  Refused like ace355_lm_decode without a prefill and at length ==
 * max_positions, and for B < 1 or n_seqs % B != 0, before anything is launched and with the handle unchanged. */
int ace355_lm_decode_tokens(ace355_lm* h, const int64_t* tokens_dev, int B, float* logits_dev, void* stream);
/* How many out-of-range tokens ace355_lm_decode_tokens has replaced since the last call of this function.  Read and cleared on the
 * stream of the last ace355_lm_decode_tokens call, with one synchronisation of that stream.  0 when that call was never made;
 * < 0 for a null handle or a HIP error. */
int64_t ace355_lm_bad_tokens(ace355_lm* h);
/* Cache fan-out: after a prefill (and any decode steps that followed it) the handle holds n_old sequences of length L; afterwards it
 * holds n_new sequences of length L, and sequence n has the K and V rows [0, L) of every layer and kv head of old sequence src[n]
 * (its stored pad rows below first[src[n]] included: the decode attention reads them, masked) and that sequence's first - as if every
 * read happened before any write.  B songs that share one prompt are prefilled once,
 * as the [2, P] CFG pair, and fanned out with src = [0] * B + [1] * B.  The copy is in place (no scratch): one launch per wave of
 * ace355_lm_fan_out_plan, in wave order, plus one tiny launch for first; stream-ordered on `stream`, which must be the stream of the
 * calls around it, and without a host synchronisation.  src host int32 [n_new] is read before the call returns.
 * ACE355_ERR_INVALID before any launch, with the handle unchanged: without a prefill, n_new outside 1 .. max_seqs, src decreasing,
 * src[n] outside [0, n], src[n] >= n_old. */
int ace355_lm_fan_out(ace355_lm* h, const int32_t* src_host, int n_new, void* stream);
/* The launch order of ace355_lm_fan_out as data (plan_lm_fan_out, csrc/lm_plan.h): wave_out[n] = the wave in which destination n is
 * written, -1 for a sequence that stays (src[n] == n); *n_waves_out = launches.  No wave reads a sequence that the same or an earlier
 * wave writes.  A pure function of src and n_old - no GPU, no handle; refuses what ace355_lm_fan_out refuses of src, with
 * 1 .. ACE355_LM_MAX_SEQS in place of max_seqs. */
int ace355_lm_fan_out_plan(const int32_t* src, int n_new, int n_old, int32_t* wave_out, int32_t* n_waves_out);

/* ------------------------------------------------------------------------------------------
 * Audio-token detokenizer of the LM-hint path: AudioTokenDetokenizer.forward,
 * base.py:886-994, as called by _decode_audio_codes_to_latents (handler/audio_codes.py:49-66) and by
 * prepare_condition (base.py:1646-1647).  Input = the quantizer's output for the 5 Hz audio codes, output =
 * lm_hints_25Hz.
 * ---------------------------------------------------------------------------------------- */
typedef struct ace355_detok ace355_detok;

typedef struct ace355_detok_config {
    int32_t hidden_size;        /* 2048 */
    int32_t intermediate_size;  /* 6144 */
    int32_t num_heads;          /* 16 */
    int32_t num_kv_heads;       /* 8 */
    int32_t head_dim;           /* 128 (only value supported) */
    int32_t num_layers;         /* 2 (num_attention_pooler_hidden_layers) */
    int32_t pool_window_size;   /* 5: 25 Hz frames per 5 Hz token */
    int32_t out_dim;            /* 64 (audio_acoustic_hidden_dim) */
    int32_t sliding_window;     /* 128 */
    uint64_t sliding_layer_mask;
    float rms_norm_eps;
    float rope_theta;
} ace355_detok_config;

int ace355_detok_create(const ace355_detok_config* cfg, ace355_detok** out);
void ace355_detok_destroy(ace355_detok* h);
/* name = a key of AudioTokenDetokenizer.state_dict() (`model.detokenizer` of the reference checkpoint). */
int ace355_detok_load_tensor(ace355_detok* h, const char* name, const void* data, int dtype, int64_t numel, int is_device);
int ace355_detok_finalize(ace355_detok* h);
/* x dev f32 [B, T5, hidden] -> out dev f32 [B, T5 * pool_window_size, out_dim]. */
int ace355_detok_run(ace355_detok* h, const float* x_dev, int B, int T5, float* out_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Audio tokenizer, the opposite direction of the same row: AceStepAudioTokenizer.forward up to its quantizer
 * (base.py:1181-1218) = audio_acoustic_proj (Linear 64 -> hidden) + AttentionPooler (base.py:734-859: embed_tokens, one
 * special token in front of every window of pool_window_size frames, num_layers encoder layers over the (B T5) sequences
 * of pool_window_size + 1 tokens, norm, token 0).  Replaces `self.tokenizer(x)` of model.tokenize (base.py:1580-1591), which
 * prepare_condition reaches for cover tasks without precomputed hints (base.py:1645).  The ResidualFSQ behind the pooler
 * (third-party vector_quantize_pytorch: Linear hidden -> 6, bounded rounding, Linear 6 -> hidden) stays with the caller
 * (ace355/lmhints.py).  Same configuration fields as the detokenizer; `out_dim` is the acoustic width (64).
 * ---------------------------------------------------------------------------------------- */
typedef struct ace355_tok ace355_tok;
typedef ace355_detok_config ace355_tok_config;
int ace355_tok_create(const ace355_tok_config* cfg, ace355_tok** out);
void ace355_tok_destroy(ace355_tok* h);
/* name = a key of AceStepAudioTokenizer.state_dict() (`model.tokenizer`) outside `quantizer.`: "audio_acoustic_proj.*",
 * "attention_pooler.*". */
int ace355_tok_load_tensor(ace355_tok* h, const char* name, const void* data, int dtype, int64_t numel, int is_device);
int ace355_tok_finalize(ace355_tok* h);
/* x dev f32 [B, T5 * pool_window_size, out_dim] (25 Hz frames, whole windows) -> out dev f32 [B, T5, hidden]. */
int ace355_tok_run(ace355_tok* h, const float* x_dev, int B, int T5, float* out_dev, void* stream);

/* The two projections of the residual FSQ quantizer on the LM-hint path (`model.tokenizer.quantizer.project_in / project_out`:
 * hidden -> 6 and 6 -> hidden; reached from H/audio_codes.py:47-66 `_decode_audio_codes_to_latents` through
 * `quantizer.get_output_from_indices`, and from base.py:1206-1218 `AceStepAudioTokenizer.forward`): out f32 [M, N] = x f32 [M, K] W^T
 * (W f32 [N, K], nn.Linear layout) + b (f32 [N] or NULL), accumulated in fp64 - the caller rounds project_in's result to FSQ digits, so a
 * half-way value must not depend on a summation order.  All pointers device memory. */
int ace355_linear_f32(const float* x_dev, const float* w_dev, const float* b_dev, float* out_dev, int64_t M, int N, int K, void* stream);

/* Post-decode peak clip, H/generate_music_decode.py:191-195: per item, if any peak > 1 divide
 * every item by clamp(peak, min=1).  wav dev f32 [B, per_item]. */
int ace355_peak_normalize(float* wav_dev, int B, int64_t per_item, void* stream);
/* NaN/Inf/all-zero latent guard, H/generate_music_decode.py:66-77: flags_host[0]=has_nan_or_inf, [1]=all_zero. */
int ace355_latent_check(const float* lat_dev, int64_t numel, int32_t* flags_host, void* stream);

/* ------------------------------------------------------------------------------------------
 * Output stage: what acestep/inference.py:649-726 does per item after the decode,
 * batched.  Replaces normalize_audio (acestep/audio_utils.py:24-62) and AudioSaver.save_audio / save_batch
 * (audio_utils.py:65-215, 259-313) for the formats whose codecs are containers over PCM: "flac" (PCM_16, the
 * reference default), "wav" / "wav32" (IEEE float32, what torchaudio's soundfile backend writes for a float32
 * tensor).  "mp3" / "opus" / "aac" go through ffmpeg in the reference and stay there.
 * ------------------------------------------------------------------------------------------ */
#define ACE355_AUDIO_FLAC 0      /* FLAC, 16 bits per sample */
#define ACE355_AUDIO_WAV_F32 1   /* RIFF/WAVE, IEEE float32 ("wav" and "wav32" of the reference) */
#define ACE355_AUDIO_WAV_PCM16 2 /* RIFF/WAVE, PCM_16 */

/* normalize_audio(audio, target_db), audio_utils.py:24-62, per item and in place: peak = max|x| over the item
 * ([channels, samples] jointly); items with peak < 1e-6 are left alone; x *= fp32(10^(dB/20)) * (1 / peak) with the
 * roundings torch applies.  wav dev f32 [n_items, per_item]; peaks_host (may be NULL) receives the peaks. */
int ace355_normalize_audio(float* wav_dev, int n_items, int64_t per_item, float target_db, float* peaks_host, void* stream);
/* dev f32 [n_items, channels, samples] -> dev interleaved [n_items, samples, channels]: int16 = lrintf(x * 32767)
 * saturated (libsndfile's float -> PCM_16 rule) when as_pcm16 != 0, else float32.  channels 1 or 2.  Asynchronous. */
int ace355_audio_interleave(const float* wav_dev, int n_items, int channels, int64_t samples, void* out_dev, int as_pcm16,
                            void* stream);
/* Host-side codecs (no GPU involved).  FLAC: RFC 9639 subset - fixed 4096-sample blocks, constant / verbatim /
 * fixed-predictor subframes, partitioned Rice coding, stereo decorrelation, CRC-8/16, MD5 in STREAMINFO; frames are
 * encoded by n_threads host threads (0 = up to 16).  pcm = interleaved int16 [frames, channels], channels 1 or 2. */
int64_t ace355_flac_bound(int64_t frames, int channels);
int ace355_flac_encode_pcm16(const int16_t* pcm, int64_t frames, int channels, int sample_rate, int n_threads, uint8_t* out,
                             int64_t cap, int64_t* out_len);
/* Decoder for AudioSaver.convert_audio (audio_utils.py:217-257) and round-trip checks: <= 16 bits per sample, 1-2
 * channels; constant / verbatim / fixed / LPC subframes, Rice and Rice2 residuals; checks every CRC, and the MD5
 * when verify_md5 != 0 and STREAMINFO carries one. */
int ace355_flac_info(const uint8_t* data, int64_t size, int64_t* frames, int32_t* channels, int32_t* sample_rate,
                     int32_t* bits_per_sample);
int ace355_flac_decode_pcm16(const uint8_t* data, int64_t size, int16_t* pcm_out, int64_t cap_samples, int verify_md5);
/* RIFF/WAVE: interleaved float32 (is_float != 0; format tag 3 + `fact` chunk) or int16 PCM. */
int64_t ace355_wav_bound(int64_t frames, int channels, int is_float);
int ace355_wav_encode(const void* interleaved, int64_t frames, int channels, int sample_rate, int is_float, uint8_t* out,
                      int64_t cap, int64_t* out_len);
/* AudioSaver.save_batch for a decoded batch still in HBM: interleave (+ quantise) on the GPU, one D2H copy of the
 * converted samples, all (item, block) encode jobs on one pool of n_threads host threads, files written in parallel.
 * wav dev f32 [n_items, channels, samples]; paths[n_items]; format = ACE355_AUDIO_*.  Synchronous. */
int ace355_save_audio_batch(const float* wav_dev, int n_items, int channels, int64_t samples, int sample_rate, int format,
                            const char* const* paths, int n_threads, void* stream);

/* ------------------------------------------------------------------------------------------
 * Input stage (the producer of SURVEY.md 8f row N3): what IoAudioMixin does between the file and tiled_encode,
 * acestep/core/generation/handler/io_audio.py:18-37 (_normalize_audio_to_stereo_48k: mono duplicated :28-29, channels 0 and 1 kept
 * :31, torchaudio.transforms.Resample(sr, 48000) :33-35, clamp to [-1, 1] :37) applied to what torchaudio.load / soundfile.read
 * (:53, :78, :129) would have decoded - the raw interleaved PCM payload goes to the GPU instead and one kernel converts (libsndfile's
 * PCM -> float rule), maps channels, resamples, clamps, and leaves max|x| for is_silence (memory_utils.py:19-21).  Containers are
 * parsed and the tap table is made on the host (ace355/audio_in.py).
 * ------------------------------------------------------------------------------------------ */
#define ACE355_PCM_U8 0    /* (v - 128) / 128 */
#define ACE355_PCM_S16 1   /* v / 2^15 */
#define ACE355_PCM_S24 2   /* packed 3-byte little endian, v / 2^23 */
#define ACE355_PCM_S32 3   /* float(v), round to nearest even, / 2^31 */
#define ACE355_PCM_F32 4   /* IEEE float32 as is */

/* With g = gcd(sr, 48000): o = sr / g, n = 48000 / g, width = ceil(6 o / (min(o, n) 0.99)) (torchaudio's sinc_interp_hann,
 * lowpass_filter_width 6, rolloff 0.99).  K = taps kept per phase of the 2 width + o.  48 kHz: o = n = 1, K = width = 0. */
typedef struct ace355_audio_in_request {
    int32_t format;     /* ACE355_PCM_* */
    int32_t channels;   /* interleaved channels in the payload, >= 1 */
    int32_t o;
    int32_t n;
    int32_t K;
    int32_t width;
    int64_t frames;     /* input frames L */
} ace355_audio_in_request;

typedef struct ace355_audio_in_plan_info {
    int64_t out_frames;     /* ceil(n L / o) */
    int64_t grid;           /* workgroups: tile t owns output frames [t tile, min(out_frames, (t + 1) tile)) */
    int32_t tile;           /* output frames per workgroup */
    int32_t threads;
    int32_t span;           /* input frames a workgroup stages per channel (0 at 48 kHz) */
    int32_t table_in_lds;   /* the tap table is copied into LDS (else read from global memory) */
    int32_t lds_bytes;
    int32_t passthrough;    /* 48 kHz: no resampling */
} ace355_audio_in_plan_info;

/* The launch ace355_audio_in_run would make (csrc/audio_in_plan.h), a pure function of the request; no GPU.  ERR_INVALID with the
 * reason in ace355_last_error for a request it refuses: a format outside ACE355_PCM_*, channels < 1, a rate <= 0 (o or n), o / n
 * not sr / 48000 in lowest terms, K / width that do not fit the rate, a dense table n (2 width + o) above 2^22 taps (rates coprime
 * to 48000 have 48000 phases; they stay with the host path), frames outside 1 .. 2^36, an output above 2^31 - 1 tiles, a rate whose
 * smallest tile does not fit in LDS. */
int ace355_audio_in_plan(const ace355_audio_in_request* rq, ace355_audio_in_plan_info* out);
/* payload_dev: a device buffer of payload_bytes bytes, 4-byte aligned and allocated up to the next multiple of 4 (the kernel loads
 * dwords and picks bytes); the samples start payload_offset bytes in, at any byte alignment: frame f, channel c at
 * payload_offset + (f channels + c) sample_bytes.  first_dev i32 [n], taps_dev f32 [n][K]: per phase p the dense-table index of its
 * first kept tap (0 <= first <= 2 width + o - K) and K consecutive taps k[p][first .. first + K); both may be NULL at 48 kHz.
 * out_dev f32 [2][out_frames]: output frame j = b n + p is clamp(sum_i taps[p][i] x[b o + first[p] + i - width], -1, 1), x zero
 * outside [0, L), accumulated in fp32 in tap order.  peak_dev f32 [1] = max|out| (a NaN in the output makes it NaN).  Enqueued on
 * `stream`; the same call gives the same bits. */
int ace355_audio_in_run(const ace355_audio_in_request* rq, const void* payload_dev, int64_t payload_bytes, int64_t payload_offset,
                        const int32_t* first_dev, const float* taps_dev, float* out_dev, float* peak_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * FLAC frames decoded on the GPU (csrc/flac_in.hip): the file's bytes go up as they are, the host walks the frame headers once
 * (ace355_flac_index), and the launches of ace355_flac_in_plan decode every frame into the interleaved PCM payload
 * ace355_audio_in_run reads.  16 to 24 bits per sample, 1 or 2 channels, every subframe form of RFC 9639 (constant, verbatim, fixed
 * orders 0-4, LPC orders 1-32, Rice and Rice2 residuals, escaped partitions, wasted bits, the four channel assignments).  Every
 * frame's CRC-16 is checked on the device; the STREAMINFO MD5 is not.
 * ------------------------------------------------------------------------------------------ */
#define ACE355_FLAC_OK 0
#define ACE355_FLAC_HEADER_MISMATCH 1 /* no sync, CRC-8, a field that differs from the frame's table row or STREAMINFO, a range that holds more than the frame */
#define ACE355_FLAC_RESERVED 2        /* a reserved or invalid code */
#define ACE355_FLAC_OVERRUN 3         /* the frame ran past its byte range */
#define ACE355_FLAC_SAMPLE_COUNT 4    /* a subframe that does not produce the block's sample count */
#define ACE355_FLAC_CRC16 5

typedef struct ace355_flac_stream_info {
    int64_t total_samples;    /* per channel */
    int64_t first_frame;      /* byte offset of the first frame */
    int32_t channels;
    int32_t bits_per_sample;
    int32_t sample_rate;
    int32_t min_block;
    int32_t max_block;
    int32_t variable_blocks;  /* the first frame's blocking-strategy bit: frame headers carry sample numbers */
} ace355_flac_stream_info;

typedef struct ace355_flac_in_plan_info {
    int64_t entropy_grid;     /* workgroups of one wave; the first entropy_lanes lanes of each own one frame */
    int64_t restore_grid;     /* the same over frames x channels subframes */
    int64_t finish_grid;      /* frames x finish_tiles workgroups: one lane per sample */
    int64_t desc_at;          /* scratch: int32 [channels][total] | subframe descriptors at desc_at | (status, assignment) per frame at frame_at */
    int64_t frame_at;
    int64_t scratch_bytes;
    int64_t out_bytes;        /* a multiple of 4 */
    int32_t launches;         /* entropy, restore, finish, status */
    int32_t entropy_threads;
    int32_t entropy_lanes;
    int32_t restore_threads;
    int32_t restore_lanes;
    int32_t finish_threads;
    int32_t finish_tiles;
    int32_t status_threads;   /* one workgroup */
    int32_t out_format;       /* ACE355_PCM_S16 at 16 bits; ACE355_PCM_S32 above, left-justified: v << (32 - bits) */
    int32_t reserved;
} ace355_flac_in_plan_info;

/* Host, no GPU.  Parses the metadata, then walks the stream once without decoding subframes: table[f] = (byte offset, byte length,
 * first sample, block size) of frame f, int64 [capacity][4]; *n_frames = the frames found, also when that exceeds capacity (ERR_INVALID
 * then: call again with a larger table).  A frame ends where the next header is found: a 0xFF 0xF8/0xF9 pair whose header parses, whose
 * CRC-8 matches, whose rate, sample size and channels agree with STREAMINFO, whose blocking bit equals the first frame's and whose coded
 * number is the expected next one; the last frame ends with the file.  CRC-16 is left to the device, so a false sync that passes all of
 * that splits a frame and shows up as that frame's status.  ERR_INVALID with the reason in ace355_last_error for: bits per sample outside
 * 16 .. 24, more than 2 channels, a STREAMINFO max block outside 16 .. 16384, an unknown (0) total sample count, block sizes that do not
 * sum to it, more than 2^24 frames.  *info is filled whenever the metadata parsed. */
int ace355_flac_index(const uint8_t* data, int64_t size, ace355_flac_stream_info* info, int64_t* table, int64_t capacity, int64_t* n_frames);
/* The launches ace355_flac_in_decode makes (csrc/flac_in_plan.h): a pure function of its arguments, no GPU.  ERR_INVALID for n_frames
 * outside 1 .. 2^24, channels other than 1 / 2, bits outside 16 .. 24, max_block outside 16 .. 16384, total_samples outside 1 .. 2^32 or
 * not within [n_frames, n_frames x max_block]. */
int ace355_flac_in_plan(int64_t n_frames, int32_t channels, int32_t bits_per_sample, int32_t max_block, int64_t total_samples,
                        ace355_flac_in_plan_info* out);
/* file_dev: the whole file, 4-byte aligned and allocated up to the next multiple of 4.  table_dev: the index's table on the device.
 * scratch_dev (16-byte aligned, plan.scratch_bytes), out_dev (plan.out_bytes): interleaved int16, or int32 left-justified above 16 bits.
 * status_dev int32 [2]: the first frame whose status is not ACE355_FLAC_OK (-1: none) and its code; such a frame's samples are zeros.
 * Rows that point outside the file or the stream are not acted on (HEADER_MISMATCH).  Enqueued on `stream`, no synchronisation. */
int ace355_flac_in_decode(const ace355_flac_stream_info* info, const void* file_dev, int64_t file_bytes, const int64_t* table_dev, int64_t n_frames,
                          void* scratch_dev, int64_t scratch_bytes, void* out_dev, int64_t out_bytes, int32_t* status_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * FLAC frames encoded on the GPU (csrc/flac_out.hip): the interleaved int16 PCM of ace355_audio_interleave goes in, every 4096-sample
 * block becomes its frame in one workgroup, the frames are compacted per item, and what comes down is the compressed bytes.  The rules
 * are the host encoder's (ace355_flac_encode_pcm16), decision for decision and tie for tie, so the file is that encoder's file byte for
 * byte.  The MD5 of STREAMINFO is a serial hash and stays on the host (or is left zero, "not computed").  Opt-in.
 * ------------------------------------------------------------------------------------------ */
#define ACE355_SAVE_FLAC_GPU 1u      /* ace355_save_audio_batch_ex: encode FLAC frames on the GPU */
#define ACE355_SAVE_FLAC_NO_MD5 2u   /* with ACE355_SAVE_FLAC_GPU: STREAMINFO's MD5 is 16 zero bytes and no PCM is copied down */

typedef struct ace355_flac_out_plan_info {
    int64_t blocks;           /* 4096-sample blocks per item */
    int64_t units;            /* n_items x blocks */
    int64_t frame_grid;       /* one workgroup per (item, block) */
    int64_t offsets_grid;     /* one workgroup per item */
    int64_t gather_grid;      /* one workgroup per (item, block) */
    int64_t item_stride;      /* output: item i's file starts at i x item_stride (ace355_flac_bound up to a multiple of 16) */
    int64_t sizes_at;         /* scratch: frame slots [units][slot_stride] | uint32 sizes [units] at sizes_at | int64 offsets [units] at offsets_at */
    int64_t offsets_at;
    int64_t scratch_bytes;
    int64_t out_bytes;
    int64_t records_bytes;    /* int64 [n_items][4]: frame bytes, smallest frame, largest frame, status (0 = fine) */
    int32_t launches;         /* frame, offsets, gather */
    int32_t frame_threads;
    int32_t offsets_threads;
    int32_t gather_threads;
    int32_t frame_lds_bytes;
    int32_t offsets_lds_bytes;
    int32_t slot_stride;      /* bytes of a frame's slot: 4096 x 2 x 17 / 8 + 64 */
    int32_t reserved;
} ace355_flac_out_plan_info;

/* The launches ace355_flac_out_encode makes (csrc/flac_out_plan.h): a pure function of its arguments, no GPU.  ERR_INVALID for n_items
 * outside 1 .. 4096, channels other than 1 / 2, frames outside 1 .. 2^36 - 1 (an empty stream is its 42 header bytes: nothing to launch),
 * n_items x blocks above 2^21. */
int ace355_flac_out_plan(int32_t n_items, int64_t frames, int32_t channels, ace355_flac_out_plan_info* out);
/* pcm_dev: interleaved int16 [n_items][frames][channels], 4-byte aligned.  scratch_dev, out_dev 16-byte aligned and at least as large as
 * the plan says; records_dev int64 [n_items][4].  Afterwards item i's frames are the records[i][0] bytes at out_dev + i x item_stride + 42;
 * the 42 bytes ahead of them are the caller's (ace355_flac_streaminfo with records[i][1], records[i][2]).  A non-zero records[i][3] means
 * a frame did not fit and the item's bytes are not a stream (it cannot happen: a frame never outgrows its verbatim form).  Enqueued on
 * `stream`, no synchronisation; the same input gives the same bytes. */
int ace355_flac_out_encode(const int16_t* pcm_dev, int32_t n_items, int64_t frames, int32_t channels, int32_t sample_rate, void* scratch_dev,
                           int64_t scratch_bytes, void* out_dev, int64_t out_bytes, int64_t* records_dev, void* stream);
/* Host: "fLaC" and the STREAMINFO block of a 16-bit stream of 4096-sample blocks, 42 bytes.  md5_or_null NULL: 16 zero bytes. */
int ace355_flac_streaminfo(uint8_t* out42, int64_t frames, int32_t channels, int32_t sample_rate, uint32_t min_frame, uint32_t max_frame,
                           const uint8_t* md5_or_null);
/* ace355_save_audio_batch with flags (ACE355_SAVE_*; ace355_save_audio_batch is this call with flags 0).  ACE355_SAVE_FLAC_GPU, FLAC
 * only (the WAV formats ignore both flags): interleave, ace355_flac_out_encode, the records and then the compressed bytes copied down,
 * STREAMINFO and the files written by the host.  The MD5 is computed by one host thread per item on a PCM copy that comes down beside the
 * encode - the files are then the flag-off files byte for byte - unless ACE355_SAVE_FLAC_NO_MD5 leaves it zero and the PCM on the GPU.
 * If the plan refuses the request, or a launch, copy or allocation fails, the files are made by the host path; ace355_last_error then
 * holds the reason, and is empty after a call that took the GPU path.  ACE355_FLAC_OUT_MAX_UNITS (environment, 1 .. 2^21) lowers the
 * plan's ceiling on n_items x blocks, each of which takes 17 KB of the scratch this call keeps.  ERR_INVALID for an unknown flag bit. */
int ace355_save_audio_batch_ex(const float* wav_dev, int n_items, int channels, int64_t samples, int sample_rate, int format,
                               const char* const* paths, int n_threads, uint32_t flags, void* stream);

/* ------------------------------------------------------------------------------------------
 * Unit kernels (test hooks; each has an oracle twin in oracle/ used by tests/)
 * ---------------------------------------------------------------------------------------- */
/* C = A[M,K] * W[N,K]^T, bf16 in, fp32 accumulate (MFMA).  out_dtype: ACE355_DTYPE_*; bias f32 [N] or NULL. */
int ace355_gemm_bf16(const void* A_dev, const void* W_dev, void* C_dev, int M, int N, int K, int out_dtype,
                     const float* bias_dev, void* stream);
/* Fused epilogues used by the DiT: mode 0: H[M,N] (f32) += gate * (A W^T), gate[n] = g1[n] + g2[(m / rows_per_seq)*g2_stride + n]
 * (NULL g1 -> gate 1);  mode 1: out[M,N/2] (bf16) = silu(gate) * up with W rows interleaved [32 gate | 32 up]. */
int ace355_gemm_bf16_fused(const void* A_dev, const void* W_dev, void* out_dev, int M, int N, int K, int mode,
                           const float* g1_dev, const float* g2_dev, int g2_stride, int rows_per_seq, void* stream);
/* Residual GEMM with the whole epilogue of the DiT's o_proj / down_proj launches (gemm.hip mode 2): H[M,N] (f32) += gate * (A W^T),
 * gate as in ace355_gemm_bf16_fused mode 0, plus cvec[n] on rows m >= cvec_row0 (the constant cross-attention term of the CFG
 * null branch: the o_proj step of csrc/dit_plan.h's pass plan).  cvec NULL: none. */
int ace355_gemm_bf16_residual(const void* A_dev, const void* W_dev, float* H_dev, int M, int N, int K, const float* g1_dev,
                              const float* g2_dev, int g2_stride, int rows_per_seq, const float* cvec_dev, int cvec_row0,
                              void* stream);
/* Projection GEMM with q / k head RMSNorm (+ RoPE when rope != 0) in its epilogue (gemm.hip mode 4; base.py:304, 338-343):
 * columns [0, q_cols) are q heads (norm weight wq [128]), [q_cols, qk_cols) k heads (wk), the rest pass through (v).
 * W bf16 [N,K] in the REFERENCE's row order; with rope the hook packs q / k rows into the library's head-pair order and the
 * q / k output columns of a head come back in that order too: dims (d, d+64) in columns (2d, 2d+1).  pos = row % rows_per_seq. */
int ace355_gemm_bf16_headnorm(const void* A_dev, const void* W_dev, void* out_bf16_dev, int M, int N, int K, int q_cols,
                              int qk_cols, const float* wq_dev, const float* wk_dev, float eps, int rope, int rows_per_seq,
                              float theta, void* stream);
/* OCP MXFP8 (gfx950 v_mfma_scale_f32_32x32x64_f8f6f4; BASELINE configs[4] "fp8 MFMA"; the reference's counterpart is torchao
 * fp8 on the DiT Linears, handler/init_service_loader.py:89-113).  mx_quantize: x bf16 [M,K] -> q fp8 e4m3 [M,K] + E8M0 block scales
 * (one per 32 consecutive K elements of a row) as uint32 [K/128][rows_pad]: byte b of word [kt][row] = block 4 kt + b;
 * rows_pad = ace355_mx_rows_pad(M).  gemm_mxfp8 (test hook): quantises both bf16 operands and runs the MX GEMM with the bf16 kernel's
 * epilogues: mode 0 out bf16 [M,N]; mode 2 H f32 [M,N] += gate * (A W^T) as ace355_gemm_bf16_fused mode 0; mode 3 SwiGLU -> bf16 [M,N/2].
 * K % 128 == 0, N % 256 == 0. */
int ace355_mx_quantize(const void* x_bf16_dev, int M, int K, void* q_out_dev, uint32_t* scales_out_dev, int rows_pad, void* stream);
int ace355_mx_rows_pad(int rows);
int ace355_gemm_mxfp8(const void* A_bf16_dev, const void* W_bf16_dev, void* out_dev, int M, int N, int K, int mode, const float* g1_dev,
                      const float* g2_dev, int g2_stride, int rows_per_seq, void* stream);
/* y = bf16( rmsnorm(x; w, eps) * (1 + sc) + sh ), sc[n] = sc1[n] + sc2[(m / rows_per_seq)*stride + n] (NULL -> no modulation). */
int ace355_rmsnorm_mod(const float* x_dev, const float* w_dev, void* y_bf16_dev, int M, int D, float eps,
                       const float* sc1, const float* sc2, const float* sh1, const float* sh2, int stride,
                       int rows_per_seq, void* stream);
/* In-place head RMSNorm (+ RoPE when rope != 0) on `heads` heads of 128 starting at column col0 of a bf16 [M, ld] matrix. */
int ace355_headnorm_rope(void* x_bf16_dev, int M, int ld, int col0, int heads, const float* w_dev, float eps,
                         int rope, int S, float theta, void* stream);
/* Flash attention: q bf16 [N,Sq,Hq*128] (ld = Hq*128), k bf16 [N,Skv,Hkv*128], v bf16 [N,Skv,Hkv*128];
 * window < 0 = full, else |i-j| <= window.  out bf16 [N,Sq,Hq*128]. */
int ace355_attention(const void* q_dev, const void* k_dev, const void* v_dev, void* out_dev, int N, int Sq, int Skv,
                     int Hq, int Hkv, int window, float scale, void* stream);
/* Cross-attention probabilities (the kernel behind ace355_dit_cross_attention_maps): q bf16 [N*Sq, q_ld] (head h at column 128 h),
 * k bf16 [N*Skv, k_ld] (KV head g at column 128 g); for the n_heads query heads heads_host[], out f32 [n_heads][N][Skv][Sq] =
 * softmax over the keys of scale q.k in fp32.  q_ld, k_ld multiples of 8, pointers 16-byte aligned; enqueued on `stream`. */
int ace355_cross_attention_probs(const void* q_dev, const void* k_dev, float* out_dev, int N, int Sq, int Skv, int Hq, int Hkv,
                                 int q_ld, int k_ld, const int32_t* heads_host, int n_heads, float scale, void* stream);
/* Same with the key-padding mask of the condition encoders (create_4d_mask, base.py:117-124, prefix form): keys
 * j >= kv_len_host[n] are masked; a query with no valid key attends uniformly to ALL keys, as the reference's
 * finfo.min additive mask does. */
int ace355_attention_masked(const void* q_dev, const void* k_dev, const void* v_dev, void* out_dev, int N, int Sq, int Skv,
                            int Hq, int Hkv, int window, float scale, const int32_t* kv_len_host, void* stream);
/* One guidance + Euler step (base.py:1946-1979): v dev f32 [2B,T,64] (cond | uncond), avg dev f32 [B,T,64]
 * momentum state (updated), xt dev f32 [B,T,64] (updated in place). first != 0: momentum buffer is empty. */
int ace355_apg_euler_step(const float* v_dev, float* avg_dev, float* xt_dev, int B, int T, float guidance, float dt,
                          int apply_cfg, int first, void* stream);
/* NLC conv (test hook for the VAE kernels): y[b,l,co] = bias[co] + sum_{tap,ci} f(x[b, l+(tap-center)*dil, ci]) * w[co,tap,ci]
 * (+ res[b,l,co]); f = snake(alpha,beta) when alpha != NULL.  x,y,res bf16 NLC; w bf16 [Cout,taps,Cin]. */
int ace355_conv1d_nlc(const void* x_dev, const void* w_dev, const float* bias_dev, const float* alpha_dev,
                      const float* beta_dev, const void* res_dev, void* y_dev, int B, int L, int Cin, int Cout,
                      int taps, int dilation, void* stream);

/* ---- Lyric alignment after the maps (align_post.hip): what MusicStampsAligner / MusicLyricScorer do on the host, on the maps as
 * ace355_dit_cross_attention_maps wrote them: maps dev f32 [n_pairs][N][L][S]; item n; lyric rows [row0, row0 + rows).  round_bf16 != 0
 * rounds every map value to bf16 and back on load (the handlers' cast to the host dtype).  Everything is enqueued on `stream`; nothing is
 * allocated: `ws` is a device workspace of at least ace355_align_workspace_bytes(n_pairs, rows, S, batch) bytes (the largest need of the
 * four calls below for those sizes; pass 1 for a size a call does not take).  The same call gives the same bits.
 * Limits: n_pairs <= 64, rows <= 8192, S <= 16384, batch <= 64, medfilt_width odd and <= 31.  ERR_INVALID, nothing enqueued: a null
 * pointer, rows < 1, S < 1, a row range outside [0, L), n outside [0, N), an even or oversized medfilt_width, a shape over the limits, a
 * workspace that is too small. */
size_t ace355_align_workspace_bytes(int n_pairs, int rows, int S, int batch);
/* MusicStampsAligner._apply_bidirectional_consensus: p = softmax_S * softmax_rows; relu(p - v median_S p); relu(p - v median_rows p);
 * p^2; energy = mean over pairs; z-score with the population mean / std of the whole block; median filter of width w along S (reflect
 * padding; the identity when S <= w / 2); calc = mean over pairs.  Medians are torch.quantile(q = 0.5) exactly; means and the std
 * accumulate in fp64.  calc, energy dev f32 [rows][S]. */
int ace355_align_timestamp_matrix(const float* maps_dev, int n_pairs, int N, int L, int S, int n, int row0, int rows, float violence_level,
                                  int medfilt_width, int round_bf16, float* calc_dev, float* energy_dev, void* ws, size_t ws_bytes,
                                  void* stream);
/* MusicLyricScorer._preprocess_attention: mean over pairs, median filter, min-max normalisation (zeros when max - min <= 1e-9) ->
 * energy; calc = energy^2. */
int ace355_align_score_matrix(const float* maps_dev, int n_pairs, int N, int L, int S, int n, int row0, int rows, int medfilt_width,
                              int round_bf16, float* calc_dev, float* energy_dev, void* ws, size_t ws_bytes, void* stream);
/* dtw_cpu + _backtrace on x = sign * m for `batch` matrices m dev f32 [batch][rows][S]: fp32 cost table, predecessor diagonal if
 * c0 < c1 && c0 < c2, else up if c1 < c0 && c1 < c2, else left; one workgroup per matrix on anti-diagonals, each cell the sequential
 * code's arithmetic.  path dev i32 [batch][2][rows + S] (row 0 lyric rows, row 1 frames), right-aligned: the last path_len[b] entries;
 * token_frames dev i32 [batch][rows][2]: the first and last frame of each lyric row on the path, -1 for a row the path skips. */
int ace355_align_dtw(const float* m_dev, int batch, int rows, int S, float sign, int32_t* path_dev, int32_t* path_len_dev,
                     int32_t* token_frames_dev, void* ws, size_t ws_bytes, void* stream);
/* MusicLyricScorer._compute_alignment_metrics in fp64 for `batch` matrices: energy dev f32 [batch][rows][S], path / path_len as
 * ace355_align_dtw wrote them, type_mask dev i32 [rows] (1 lyric, 0 tag; shared by the batch).  out dev f64 [batch][3]: coverage,
 * monotonicity, path confidence (1, 1, 0 in the empty cases). */
int ace355_align_score_metrics(const float* energy_dev, const int32_t* path_dev, const int32_t* path_len_dev, const int32_t* type_mask_dev,
                               int batch, int rows, int S, double time_weight, double overlap_frames, double instrumental_weight,
                               double* out_dev, void* ws, size_t ws_bytes, void* stream);
/* Test hook of the selection behind the medians: x dev f32 [outer][n][inner] -> out dev f32 [outer][inner], torch.quantile(x, 0.5, dim=1)
 * bit for bit.  n >= 1, inner and outer in [1, 65535]. */
int ace355_align_median(const float* x_dev, int outer, int n, int inner, float* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ACE355_H */
