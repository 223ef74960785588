// cond.hip - the encoder-stack handles behind ace355.h: the condition encoder and the audio-token
// detokenizer of the LM-hint path (row N2, AudioTokenDetokenizer, base.py:862-994, at the end of this file).  N1: weight ingestion/packing and
// AceStepConditionEncoder.forward (base.py:1509-1554) = text projector + AceStepLyricEncoder (base.py:577-731) +
// AceStepTimbreEncoder (base.py:997-1178) + two pack_sequences (base.py:138-169).  Host-side orchestration only: every
// contraction / norm / attention runs on the DiT's kernels (gemm.hip, attn.hip, elementwise.hip).
//
// Differences from the DiT layer that matter here: plain residuals (no gates), un-modulated RMSNorm, and REAL key-padding
// masks on the lyric encoder.  Padding rows are not dead data: the DiT ignores encoder_attention_mask (base.py:1384-1385),
// so the encoder outputs at padded positions flow into the DiT's cross-attention and must match the reference too -
// including query rows with no valid key on sliding layers (AttnArgs::vmean).
//
// The layer stack itself, its key map and the load / finalize / destroy bookkeeping are encoder.hip's; this file holds the three handles,
// their non-layer keys and create / encode / run.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "encoder.h"

using namespace ace355;

struct ace355_cond : EncBase {
    ace355_cond_config cfg;
    EncoderW lyric, timbre;
    bf16_t* w_text = nullptr;
    // outputs of the three branches ahead of pack_sequences, [out_rows][D] each
    bf16_t *lyric_out = nullptr, *timbre_out = nullptr, *text_out = nullptr;
    std::vector<void*> out_allocs;
    long out_rows = 0;
    int* rowsrc_dev = nullptr;
    long rowsrc_cap = 0;
};

struct ace355_detok : EncBase {
    ace355_detok_config cfg;
    EncoderW enc;            // embed_tokens / layers / norm
    float* special = nullptr;  // [pool][D]
    bf16_t* w_out = nullptr;   // [out_dim][D]
    float* b_out = nullptr;
};

// AceStepAudioTokenizer up to the quantizer (base.py:1181-1223): audio_acoustic_proj + AttentionPooler (base.py:734-859)
struct ace355_tok : EncBase {
    ace355_tok_config cfg;
    EncoderW enc;              // attention_pooler.embed_tokens / layers / norm
    float* special = nullptr;  // attention_pooler.special_token [D]
    bf16_t* w_in = nullptr;    // audio_acoustic_proj.weight [D][in_pad] (K padded to a multiple of 64)
    float* b_in = nullptr;
    int in_pad = 64;
    bf16_t* proj = nullptr;    // workspace: projected frames bf16 [R][D]
    long proj_rows = 0;
};

namespace {

// embed_tokens (Linear with bias) + final norm of an encoder, keys relative to its prefix
bool resolve_embed_norm(const EncBase& h, EncoderW& E, const std::string& r, PackDest* d) {
    const long D = h.D;
    if (r == "embed_tokens.weight") { *d = pack_rows(E.w_embed, 1, D, E.in_dim, E.in_dim, 0); return true; }
    if (r == "embed_tokens.bias") { *d = pack_rows(E.b_embed, 0, 1, D, D, 0); return true; }
    if (r == "norm.weight") { *d = pack_rows(E.norm, 0, 1, D, D, 0); return true; }
    return false;
}

// Map a key of AceStepConditionEncoder.state_dict() to its packed destination.
bool resolve(ace355_cond* h, const std::string& name, PackDest* d) {
    const long D = h->D, TD = h->cfg.text_hidden_dim;
    if (name == "text_projector.weight") { *d = pack_rows(h->w_text, 1, D, TD, TD, 0); return true; }
    for (int e = 0; e < 2; ++e) {
        const std::string p = e == 0 ? "lyric_encoder." : "timbre_encoder.";
        if (name.rfind(p, 0) != 0) continue;
        EncoderW& E = e == 0 ? h->lyric : h->timbre;
        const std::string r = name.substr(p.size());
        if (r == "special_token") {  // parameter of the reference module that its forward never reads (base.py:1015)
            *d = pack_rows(nullptr, 0, 1, D, D, 0);
            d->ignore = true;
            return true;
        }
        return resolve_embed_norm(*h, E, r, d) || resolve_encoder_layers(*h, E, name, p.size(), d);
    }
    return false;
}

// embed (Linear with bias, base.py:623 / :1070) then the layers.  in_bf: [N*S, in_dim] bf16.
int encoder_stack(EncBase* h, const EncoderW& E, const bf16_t* in_bf, const EncPassRequest& rq, const int* kv_len_dev, bf16_t* out, hipStream_t s) {
    GemmEpilogue ep{1, E.b_embed, nullptr, nullptr, 0, 0};
    int rc = launch_gemm(in_bf, E.in_dim, E.w_embed, E.in_dim, h->h, h->D, rq.N * rq.S, h->D, E.in_dim, ep, s);
    if (rc) return rc;
    return run_encoder_pass(h, E, rq, kv_len_dev, out, s);
}

// the three branch outputs, grown like the workspace
int ensure_outputs(ace355_cond* h, long rows, hipStream_t s) {
    if (rows <= h->out_rows) return 0;
    ACE_HIP(hipStreamSynchronize(s));
    for (void* p : h->out_allocs) hipFree(p);
    h->out_allocs.clear();
    h->out_rows = 0;
    ALLOC(h->out_allocs, h->lyric_out, (size_t)rows * h->D);
    ALLOC(h->out_allocs, h->timbre_out, (size_t)rows * h->D);
    ALLOC(h->out_allocs, h->text_out, (size_t)rows * h->D);
    h->out_rows = rows;
    return 0;
}

}  // namespace

extern "C" {

int ace355_cond_create(const ace355_cond_config* cfg, ace355_cond** out) {
    ACE_CHECK(cfg && out, "cond_create: null argument");
    ACE_CHECK(cfg->head_dim == 128, "cond_create: head_dim must be 128");
    ACE_CHECK(cfg->hidden_size % 256 == 0 && cfg->intermediate_size % 64 == 0, "cond_create: hidden/intermediate size");
    ACE_CHECK(cfg->text_hidden_dim % 64 == 0 && cfg->timbre_hidden_dim % 64 == 0, "cond_create: input dims must be multiples of 64");
    ACE_CHECK(cfg->num_heads % cfg->num_kv_heads == 0, "cond_create: heads % kv_heads");
    ACE_CHECK(cfg->num_lyric_layers >= 0 && cfg->num_lyric_layers <= 64 && cfg->num_timbre_layers >= 0 && cfg->num_timbre_layers <= 64,
              "cond_create: layer counts");
    ace355_cond* h = new ace355_cond();
    h->cfg = *cfg;
    enc_init(h, cfg->hidden_size, cfg->intermediate_size, cfg->num_heads, cfg->num_kv_heads, cfg->sliding_window, cfg->sliding_layer_mask,
             cfg->rms_norm_eps, cfg->rope_theta);
    int rc = dev_alloc(h->allocs, &h->w_text, (size_t)h->D * cfg->text_hidden_dim);
    if (!rc) rc = alloc_encoder(h, h->lyric, cfg->num_lyric_layers, cfg->text_hidden_dim);
    if (!rc) rc = alloc_encoder(h, h->timbre, cfg->num_timbre_layers, cfg->timbre_hidden_dim);
    if (rc) { ace355_cond_destroy(h); return rc; }
    h->expected_tensors = 1 + (3 + (size_t)cfg->num_lyric_layers * 11) + (3 + (size_t)cfg->num_timbre_layers * 11);
    *out = h;
    return ACE355_OK;
}

void ace355_cond_destroy(ace355_cond* h) {
    if (!h) return;
    hipDeviceSynchronize();
    free_encoder(h);
    for (void* p : h->out_allocs) hipFree(p);
    if (h->rowsrc_dev) hipFree(h->rowsrc_dev);
    delete h;
}

int ace355_cond_load_tensor(ace355_cond* h, const char* name, const void* data, int dtype, int64_t numel, int is_device) {
    ACE_CHECK(h && name && data, "cond_load_tensor: null argument");
    ACE_CHECK(dtype == ACE355_DTYPE_F32 || dtype == ACE355_DTYPE_BF16, "cond_load_tensor: dtype");
    PackDest d;
    if (!resolve(h, name, &d)) return unknown_tensor("cond_load_tensor", name);
    return load_packed(h, d, name, data, dtype, numel, is_device, "cond_load_tensor");
}

int ace355_cond_finalize(ace355_cond* h) {
    ACE_CHECK(h, "cond_finalize: null handle");
    return finalize_loaded(h, "cond_finalize");
}

int ace355_cond_out_len(int Ll, int Lt, const int32_t* refer_item, int Nref, int B) {
    if (Ll < 0 || Lt < 0 || Nref < 0 || B <= 0 || (Nref > 0 && !refer_item)) return -1;
    std::vector<int> cnt(B, 0);
    int mx = 0;
    for (int i = 0; i < Nref; ++i) {
        if (refer_item[i] < 0 || refer_item[i] >= B) return -1;
        mx = std::max(mx, ++cnt[refer_item[i]]);
    }
    return Ll + mx + Lt;
}

int ace355_cond_encode(ace355_cond* h, const float* text_dev, const int32_t* text_len, int Lt, const float* lyric_dev,
                       const int32_t* lyric_len, int Ll, const float* refer_dev, const int32_t* refer_item, int Nref, int Tref, int B,
                       float* enc_out_dev, int32_t* enc_len_out, void* stream) {
    ACE_CHECK(h && text_dev && text_len && lyric_dev && lyric_len && refer_dev && refer_item && enc_out_dev && enc_len_out,
              "cond_encode: null argument");
    if (!h->finalized) { set_error("cond_encode: call ace355_cond_finalize first"); return ACE355_ERR_STATE; }
    ACE_CHECK(B > 0 && B <= 64 && Lt > 0 && Ll > 0 && Nref > 0 && Nref <= 256 && Tref > 0, "cond_encode: sizes");
    hipStream_t s = (hipStream_t)stream;
    const int D = h->D, TD = h->cfg.text_hidden_dim, AD = h->cfg.timbre_hidden_dim;
    for (int b = 0; b < B; ++b) {
        ACE_CHECK(text_len[b] >= 0 && text_len[b] <= Lt && lyric_len[b] >= 0 && lyric_len[b] <= Ll, "cond_encode: lengths out of range");
    }
    std::vector<int> cnt(B, 0);
    int max_cnt = 0;
    for (int i = 0; i < Nref; ++i) {
        ACE_CHECK(refer_item[i] >= 0 && refer_item[i] < B, "cond_encode: refer_item out of range");
        max_cnt = std::max(max_cnt, ++cnt[refer_item[i]]);
    }
    const int Lout = Ll + max_cnt + Lt;
    const EncPassRequest passes[2] = {enc_request(*h, h->lyric, B, Ll, true), enc_request(*h, h->timbre, Nref, Tref)};
    const long rows = std::max<long>({(long)B * Ll, (long)Nref * Tref, (long)B * Lt});   // of the three branch outputs
    const long in_elems = std::max<long>({(long)B * Ll * TD, (long)Nref * Tref * AD, (long)B * Lt * TD});
    int rc = ensure_workspace(h, plan_encoder_workspace(passes, 2, in_elems, 0), s);
    if (!rc) rc = ensure_outputs(h, rows, s);
    if (rc) return rc;

    // text: Linear(text_dim -> D, no bias) (base.py:1541)
    rc = launch_f32_to_bf16(text_dev, h->in_bf, (long)B * Lt * TD, s);
    if (rc) return rc;
    GemmEpilogue ep{0, nullptr, nullptr, nullptr, 0, 0};
    rc = launch_gemm(h->in_bf, TD, h->w_text, TD, h->text_out, D, B * Lt, D, TD, ep, s);
    if (rc) return rc;

    // lyric encoder with its key-padding mask (base.py:1543-1547)
    rc = launch_f32_to_bf16(lyric_dev, h->in_bf, (long)B * Ll * TD, s);
    if (rc) return rc;
    ACE_HIP(hipMemcpyAsync(h->kvlen_dev, lyric_len, sizeof(int) * B, hipMemcpyHostToDevice, s));
    ACE_HIP(hipStreamSynchronize(s));  // lyric_len is caller memory
    rc = encoder_stack(h, h->lyric, h->in_bf, passes[0], h->kvlen_dev, h->lyric_out, s);
    if (rc) return rc;

    // timbre encoder: no padding mask, token 0 of every reference clip (base.py:1549, :1175)
    rc = launch_f32_to_bf16(refer_dev, h->in_bf, (long)Nref * Tref * AD, s);
    if (rc) return rc;
    rc = encoder_stack(h, h->timbre, h->in_bf, passes[1], nullptr, h->timbre_out, s);
    if (rc) return rc;

    // pack_sequences twice (base.py:1553-1554) with prefix masks = a segmented row gather per batch item:
    //   [lyric valid | timbre valid | text valid | lyric padding | timbre zero rows | text padding]
    // The three sources live in one virtual row space: lyric rows [0, B*Ll), timbre rows (token 0 of clip i) B*Ll + i,
    // text rows B*Ll + Nref + r; they are gathered from three buffers, so build three index tables and gather three times.
    const long total = (long)B * Lout;
    if (total * 3 > h->rowsrc_cap) {
        ACE_HIP(hipStreamSynchronize(s));
        if (h->rowsrc_dev) hipFree(h->rowsrc_dev);
        ACE_HIP(hipMalloc((void**)&h->rowsrc_dev, sizeof(int) * total * 3 + 256));
        h->rowsrc_cap = total * 3;
    }
    std::vector<int> src_l(total, -2), src_t(total, -2), src_x(total, -2);  // -2: row not owned by this source
    std::vector<std::vector<int>> clips(B);
    for (int i = 0; i < Nref; ++i) clips[refer_item[i]].push_back(i);
    for (int b = 0; b < B; ++b) {
        long o = (long)b * Lout;
        const int ll = lyric_len[b], tl = text_len[b], c = cnt[b];
        for (int j = 0; j < ll; ++j) src_l[o++] = b * Ll + j;
        for (int j = 0; j < c; ++j) src_t[o++] = clips[b][j] * Tref;  // token 0 of the clip
        for (int j = 0; j < tl; ++j) src_x[o++] = b * Lt + j;
        for (int j = ll; j < Ll; ++j) src_l[o++] = b * Ll + j;
        for (int j = c; j < max_cnt; ++j) src_t[o++] = -1;              // zero rows of the one-hot unpack
        for (int j = tl; j < Lt; ++j) src_x[o++] = b * Lt + j;
        enc_len_out[b] = ll + c + tl;
    }
    // compact each table to (dst row, src row) pairs handled by one gather over the owned rows only
    std::vector<int> table(total * 3);
    const std::vector<int>* tabs[3] = {&src_l, &src_t, &src_x};
    const bf16_t* bufs[3] = {h->lyric_out, h->timbre_out, h->text_out};
    for (int t = 0; t < 3; ++t) memcpy(table.data() + total * t, tabs[t]->data(), sizeof(int) * total);
    ACE_HIP(hipMemcpyAsync(h->rowsrc_dev, table.data(), sizeof(int) * total * 3, hipMemcpyHostToDevice, s));
    for (int t = 0; t < 3; ++t) {
        rc = launch_gather_rows_bf16_f32(bufs[t], D, h->rowsrc_dev + total * t, enc_out_dev, D, total, D, s);
        if (rc) return rc;
    }
    ACE_HIP(hipStreamSynchronize(s));  // `table` is host memory
    return ACE355_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ detokenizer (N2)
namespace {

bool resolve_detok(ace355_detok* h, const std::string& name, PackDest* d) {
    const long D = h->D, OD = h->cfg.out_dim;
    if (name == "special_tokens") { *d = pack_rows(h->special, 0, h->cfg.pool_window_size, D, D, 0); return true; }
    if (name == "proj_out.weight") { *d = pack_rows(h->w_out, 1, OD, D, D, 0); return true; }
    if (name == "proj_out.bias") { *d = pack_rows(h->b_out, 0, 1, OD, OD, 0); return true; }
    return resolve_embed_norm(*h, h->enc, name, d) || resolve_encoder_layers(*h, h->enc, name, 0, d);
}

}  // namespace

extern "C" {

int ace355_detok_create(const ace355_detok_config* cfg, ace355_detok** out) {
    ACE_CHECK(cfg && out, "detok_create: null argument");
    ACE_CHECK(cfg->head_dim == 128, "detok_create: head_dim must be 128");
    ACE_CHECK(cfg->hidden_size % 256 == 0 && cfg->intermediate_size % 64 == 0, "detok_create: hidden/intermediate size");
    ACE_CHECK(cfg->num_heads % cfg->num_kv_heads == 0, "detok_create: heads % kv_heads");
    ACE_CHECK(cfg->num_layers >= 0 && cfg->num_layers <= 64 && cfg->pool_window_size >= 1 && cfg->pool_window_size <= 64 &&
                  cfg->out_dim >= 1, "detok_create: layer count / pool window / out_dim");
    ace355_detok* h = new ace355_detok();
    h->cfg = *cfg;
    enc_init(h, cfg->hidden_size, cfg->intermediate_size, cfg->num_heads, cfg->num_kv_heads, cfg->sliding_window, cfg->sliding_layer_mask,
             cfg->rms_norm_eps, cfg->rope_theta);
    int rc = alloc_encoder(h, h->enc, cfg->num_layers, cfg->hidden_size);
    if (!rc) rc = dev_alloc(h->allocs, &h->special, (size_t)cfg->pool_window_size * h->D);
    if (!rc) rc = dev_alloc(h->allocs, &h->w_out, (size_t)cfg->out_dim * h->D);
    if (!rc) rc = dev_alloc(h->allocs, &h->b_out, (size_t)cfg->out_dim);
    if (rc) { ace355_detok_destroy(h); return rc; }
    h->expected_tensors = 6 + (size_t)cfg->num_layers * 11;
    *out = h;
    return ACE355_OK;
}

void ace355_detok_destroy(ace355_detok* h) {
    if (!h) return;
    hipDeviceSynchronize();
    free_encoder(h);
    delete h;
}

int ace355_detok_load_tensor(ace355_detok* h, const char* name, const void* data, int dtype, int64_t numel, int is_device) {
    ACE_CHECK(h && name && data, "detok_load_tensor: null argument");
    ACE_CHECK(dtype == ACE355_DTYPE_F32 || dtype == ACE355_DTYPE_BF16, "detok_load_tensor: dtype");
    PackDest d;
    if (!resolve_detok(h, name, &d)) return unknown_tensor("detok_load_tensor", name);
    return load_packed(h, d, name, data, dtype, numel, is_device, "detok_load_tensor");
}

int ace355_detok_finalize(ace355_detok* h) {
    ACE_CHECK(h, "detok_finalize: null handle");
    return finalize_loaded(h, "detok_finalize");
}

int ace355_detok_run(ace355_detok* h, const float* x_dev, int B, int T5, float* out_dev, void* stream) {
    ACE_CHECK(h && x_dev && out_dev, "detok_run: null argument");
    if (!h->finalized) { set_error("detok_run: call ace355_detok_finalize first"); return ACE355_ERR_STATE; }
    ACE_CHECK(B > 0 && T5 > 0 && (long)B * T5 <= (1L << 20), "detok_run: sizes");
    hipStream_t s = (hipStream_t)stream;
    const int D = h->D, P = h->cfg.pool_window_size, OD = h->cfg.out_dim;
    const long R5 = (long)B * T5, R = R5 * P;  // 5 Hz tokens, 25 Hz rows: R5 sequences of P tokens
    const EncPassRequest rq = enc_request(*h, h->enc, (int)R5, P);
    int rc = ensure_workspace(h, plan_encoder_workspace(&rq, 1, R5 * D, R5), s);
    if (rc) return rc;
    // embed_tokens (base.py:888), then one copy per frame of the window + its special token (:889-894)
    rc = launch_f32_to_bf16(x_dev, h->in_bf, R5 * D, s);
    if (rc) return rc;
    GemmEpilogue ep{1, h->enc.b_embed, nullptr, nullptr, 0, 0};
    rc = launch_gemm(h->in_bf, D, h->enc.w_embed, D, h->emb, D, (int)R5, D, D, ep, s);
    if (rc) return rc;
    rc = launch_expand_add(h->emb, h->special, h->h, R5, P, D, s);
    if (rc) return rc;
    // (b t) sequences of P tokens through the encoder layers + norm (:896-987), proj_out (:989), unfold (:991) is a view
    rc = run_encoder_pass(h, h->enc, rq, nullptr, h->xn, s);
    if (rc) return rc;
    ep = GemmEpilogue{1, h->b_out, nullptr, nullptr, 0, 0};
    return launch_gemm(h->xn, D, h->w_out, D, out_dev, OD, (int)R, OD, D, ep, s);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ audio tokenizer (N2, the other direction)
// AceStepAudioTokenizer.forward up to the quantizer (base.py:1206-1218): x [B, T5, P, 64] -> audio_acoustic_proj (Linear 64 -> D) ->
// AttentionPooler: embed_tokens (Linear D -> D), one special token in FRONT of every window of P frames, the (B T5) sequences of P + 1
// tokens through the encoder layers + norm, token 0 of each sequence is the pooled 5 Hz representation [B, T5, D].  Reached by
// prepare_condition for cover tasks without precomputed hints (base.py:1645).  The ResidualFSQ behind it is a [n, D] x [D, 6]
// product + rounding and stays with the caller (lmhints.py).
namespace {

bool resolve_tok(ace355_tok* h, const std::string& name, PackDest* d) {
    const long D = h->D;
    if (name == "audio_acoustic_proj.weight") { *d = pack_rows(h->w_in, 1, D, h->cfg.out_dim, h->in_pad, 0); return true; }
    if (name == "audio_acoustic_proj.bias") { *d = pack_rows(h->b_in, 0, 1, D, D, 0); return true; }
    const std::string p = "attention_pooler.";
    if (name.rfind(p, 0) != 0) return false;
    const std::string r = name.substr(p.size());
    if (r == "special_token") { *d = pack_rows(h->special, 0, 1, D, D, 0); return true; }
    return resolve_embed_norm(*h, h->enc, r, d) || resolve_encoder_layers(*h, h->enc, name, p.size(), d);
}

}  // namespace

extern "C" {

int ace355_tok_create(const ace355_tok_config* cfg, ace355_tok** out) {
    ACE_CHECK(cfg && out, "tok_create: null argument");
    ACE_CHECK(cfg->head_dim == 128, "tok_create: head_dim must be 128");
    ACE_CHECK(cfg->hidden_size % 256 == 0 && cfg->intermediate_size % 64 == 0, "tok_create: hidden/intermediate size");
    ACE_CHECK(cfg->num_heads % cfg->num_kv_heads == 0, "tok_create: heads % kv_heads");
    ACE_CHECK(cfg->num_layers >= 0 && cfg->num_layers <= 64 && cfg->pool_window_size >= 1 && cfg->pool_window_size <= 63 &&
                  cfg->out_dim >= 1 && cfg->out_dim <= 4096, "tok_create: layer count / pool window / acoustic dim");
    ace355_tok* h = new ace355_tok();
    h->cfg = *cfg;
    enc_init(h, cfg->hidden_size, cfg->intermediate_size, cfg->num_heads, cfg->num_kv_heads, cfg->sliding_window, cfg->sliding_layer_mask,
             cfg->rms_norm_eps, cfg->rope_theta);
    h->in_pad = ((cfg->out_dim + 63) / 64) * 64;
    int rc = alloc_encoder(h, h->enc, cfg->num_layers, cfg->hidden_size);
    if (!rc) rc = dev_alloc(h->allocs, &h->special, (size_t)h->D);
    if (!rc) rc = dev_alloc(h->allocs, &h->w_in, (size_t)h->D * h->in_pad);
    if (!rc) rc = dev_alloc(h->allocs, &h->b_in, (size_t)h->D);
    if (!rc && hipMemset(h->w_in, 0, (size_t)h->D * h->in_pad * sizeof(bf16_t)) != hipSuccess) rc = ACE355_ERR_HIP;
    if (rc) { ace355_tok_destroy(h); return rc; }
    h->expected_tensors = 6 + (size_t)cfg->num_layers * 11;
    *out = h;
    return ACE355_OK;
}

void ace355_tok_destroy(ace355_tok* h) {
    if (!h) return;
    hipDeviceSynchronize();
    free_encoder(h);
    if (h->proj) hipFree(h->proj);
    delete h;
}

int ace355_tok_load_tensor(ace355_tok* h, const char* name, const void* data, int dtype, int64_t numel, int is_device) {
    ACE_CHECK(h && name && data, "tok_load_tensor: null argument");
    ACE_CHECK(dtype == ACE355_DTYPE_F32 || dtype == ACE355_DTYPE_BF16, "tok_load_tensor: dtype");
    PackDest d;
    if (!resolve_tok(h, name, &d)) return unknown_tensor("tok_load_tensor", name);
    return load_packed(h, d, name, data, dtype, numel, is_device, "tok_load_tensor");
}

int ace355_tok_finalize(ace355_tok* h) {
    ACE_CHECK(h, "tok_finalize: null handle");
    return finalize_loaded(h, "tok_finalize");
}

int ace355_tok_run(ace355_tok* h, const float* x_dev, int B, int T5, float* out_dev, void* stream) {
    ACE_CHECK(h && x_dev && out_dev, "tok_run: null argument");
    if (!h->finalized) { set_error("tok_run: call ace355_tok_finalize first"); return ACE355_ERR_STATE; }
    ACE_CHECK(B > 0 && T5 > 0 && (long)B * T5 <= (1L << 20), "tok_run: sizes");
    hipStream_t s = (hipStream_t)stream;
    const int D = h->D, P = h->cfg.pool_window_size, A = h->cfg.out_dim, S = P + 1;
    const long R5 = (long)B * T5, R = R5 * P;  // 5 Hz tokens = sequences of S = P + 1 tokens, 25 Hz frames
    const EncPassRequest rq = enc_request(*h, h->enc, (int)R5, S);
    int rc = ensure_workspace(h, plan_encoder_workspace(&rq, 1, R * h->in_pad, R), s);
    if (rc) return rc;
    if (R > h->proj_rows) {
        ACE_HIP(hipStreamSynchronize(s));
        if (h->proj) hipFree(h->proj);
        h->proj = nullptr; h->proj_rows = 0;
        ACE_HIP(hipMalloc((void**)&h->proj, (size_t)R * D * sizeof(bf16_t) + 256));
        h->proj_rows = R;
    }
    // frames -> bf16 rows of in_pad columns (zero beyond the acoustic width), audio_acoustic_proj (base.py:1213), embed_tokens (:768)
    rc = launch_pad_rows_bf16(x_dev, h->in_bf, R, A, h->in_pad, s);
    if (rc) return rc;
    GemmEpilogue ep{0, h->b_in, nullptr, nullptr, 0, 0};
    rc = launch_gemm(h->in_bf, h->in_pad, h->w_in, h->in_pad, h->proj, D, (int)R, D, h->in_pad, ep, s);
    if (rc) return rc;
    ep = GemmEpilogue{1, h->enc.b_embed, nullptr, nullptr, 0, 0};
    rc = launch_gemm(h->proj, D, h->enc.w_embed, D, h->emb, D, (int)R, D, D, ep, s);
    if (rc) return rc;
    // [special | P frames] per window (:769-771), the (b t) sequences through the layers + norm (:773-853), token 0 of each (:856-858)
    rc = launch_prepend_special(h->emb, h->special, h->h, R5, P, D, s);
    if (rc) return rc;
    rc = run_encoder_pass(h, h->enc, rq, nullptr, h->xn, s);
    if (rc) return rc;
    return launch_take_token0(h->xn, out_dev, R5, S, D, s);
}

}  // extern "C"
