// audio_in.hip - the input stage ahead of the VAE encoder (SURVEY.md 8f row N3's producer):
//   acestep/core/generation/handler/io_audio.py:18-37 (_normalize_audio_to_stereo_48k) on the samples as they sit in the file.
// The reference decodes on the host (torchaudio / soundfile -> libsndfile), resamples with a dense strided fp32 conv1d on host threads,
// clamps, and copies the result to the GPU.  Here the RAW interleaved payload goes up once and one kernel does the rest: libsndfile's
// PCM -> float rule per sample, the channel map (mono duplicated, channels 0 and 1 of anything wider), torchaudio's polyphase resampler
// with only the taps that carry weight, the clamp in the store, and max|x| of the result for is_silence (memory_utils.py:19-21).
// One workgroup per tile of output frames (audio_in_plan.h): it converts the tile's input span once into LDS for both channels, then
// output frame j = b n + p is the K taps of phase p over LDS floats [b o + first[p], + K), accumulated in fp32 in tap order.  Lane l
// of a wave owns output l of 64 consecutive ones, so the LDS reads of a wave are ~1 float apart (x) and K | 1 floats apart (taps): no
// bank conflicts at odd strides, and a wave's store is 256 contiguous bytes per channel.  No float atomics: the peak is an integer
// max on the bit pattern of |x| (IEEE order = integer order for non-negative floats; a NaN sorts above everything and survives, as
// it does in torch.max), so the same call gives the same bits.
#include "../../include/ace355.h"
#include "audio_in_plan.h"
#include "common.h"

namespace ace355 {
namespace {

struct AudioInArgs {
    const uint32_t* words;      // the payload buffer as dwords (base 4-byte aligned; samples are not)
    long long byte0;            // byte offset of frame 0, channel 0
    const int32_t* first;       // [n]
    const float* taps;          // [n][K]
    float* out;                 // [2][out_frames]
    uint32_t* peak_bits;        // [1], zeroed ahead of the launch
    long long frames, out_frames;
    int channels, o, n, K, width, tile, span, table_in_lds;
};

// One sample at any byte address: the dword that holds its first byte, and the next one when it straddles.
template <int FMT>
__device__ __forceinline__ float pcm_load(const uint32_t* __restrict__ w, long long byte) {
    constexpr int BITS = FMT == ACE355_PCM_U8 ? 8 : FMT == ACE355_PCM_S16 ? 16 : FMT == ACE355_PCM_S24 ? 24 : 32;
    const long long d = byte >> 2;
    const int sh = (int)(byte & 3) * 8;
    uint32_t v = w[d] >> sh;
    if (sh + BITS > 32) v |= w[d + 1] << (32 - sh);   // (sh >= 8 here)
    if (FMT == ACE355_PCM_U8) return (float)((int)(v & 0xffu) - 128) * 0.0078125f;
    if (FMT == ACE355_PCM_S16) return (float)(int16_t)(v & 0xffffu) * 3.0517578125e-05f;
    if (FMT == ACE355_PCM_S24) return (float)((int32_t)(v << 8) >> 8) * 1.1920928955078125e-07f;
    if (FMT == ACE355_PCM_S32) return (float)(int32_t)v * 4.656612873077393e-10f;   // the conversion rounds to nearest even; 2^-31 is exact
    return __uint_as_float(v);
}

// torch.clamp(x, -1, 1): a NaN stays a NaN
__device__ __forceinline__ float clamp1(float x) { return x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x); }

template <int FMT>
__global__ __launch_bounds__(AUDIO_IN_THREADS) void audio_in_kernel(const AudioInArgs a) {
    extern __shared__ float smem[];
    __shared__ uint32_t wave_peak[AUDIO_IN_THREADS / 64];
    constexpr int BYTES = FMT == ACE355_PCM_U8 ? 1 : FMT == ACE355_PCM_S16 ? 2 : FMT == ACE355_PCM_S24 ? 3 : 4;
    const int tid = threadIdx.x;
    const long long j0 = (long long)blockIdx.x * a.tile;
    const long long left = a.out_frames - j0;
    const int count = left < a.tile ? (int)left : a.tile;
    const int c1 = a.channels == 1 ? 0 : 1;
    float* __restrict__ out0 = a.out + j0;
    float* __restrict__ out1 = a.out + a.out_frames + j0;
    uint32_t peak = 0;
    if (a.K == 0) {   // 48 kHz: the conversion rule, the channel map and the clamp
        for (int r = tid; r < count; r += AUDIO_IN_THREADS) {
            const long long at = a.byte0 + (j0 + r) * a.channels * BYTES;
            const float x0 = clamp1(pcm_load<FMT>(a.words, at));
            const float x1 = c1 ? clamp1(pcm_load<FMT>(a.words, at + BYTES)) : x0;
            out0[r] = x0, out1[r] = x1;
            const uint32_t b0 = __float_as_uint(x0) & 0x7fffffffu, b1 = __float_as_uint(x1) & 0x7fffffffu;
            peak = max(peak, max(b0, b1));
        }
    } else {
        float* xs0 = smem;
        float* xs1 = smem + a.span;
        const int kp = a.K | 1;
        const int32_t* first = a.first;
        const float* taps = a.taps;
        int tstride = a.K;
        if (a.table_in_lds) {
            int32_t* lfirst = reinterpret_cast<int32_t*>(smem + 2 * a.span);
            float* ltaps = smem + 2 * a.span + a.n;
            for (int i = tid; i < a.n; i += AUDIO_IN_THREADS) lfirst[i] = a.first[i];
            for (int i = tid; i < a.n * a.K; i += AUDIO_IN_THREADS) ltaps[(i / a.K) * kp + i % a.K] = a.taps[i];
            first = lfirst, taps = ltaps, tstride = kp;
        }
        const long long b0 = j0 / a.n;
        const int jj0 = (int)(j0 - b0 * a.n);
        const long long s0 = b0 * a.o - a.width;   // the input frame LDS slot 0 holds
        for (int idx = tid; idx < 2 * a.span; idx += AUDIO_IN_THREADS) {
            const int i = idx >> 1, c = idx & 1;
            const long long f = s0 + i;
            float v = 0.0f;
            if (f >= 0 && f < a.frames) v = pcm_load<FMT>(a.words, a.byte0 + (f * a.channels + (c ? c1 : 0)) * BYTES);
            (c ? xs1 : xs0)[i] = v;
        }
        __syncthreads();
        const int fmax = 2 * a.width + a.o - a.K;
        for (int r = tid; r < count; r += AUDIO_IN_THREADS) {
            const int jj = jj0 + r, bl = jj / a.n, p = jj - bl * a.n;
            const int at = bl * a.o + min(max(first[p], 0), fmax);   // (the clamp keeps a corrupt table inside the staged span)
            const float* __restrict__ k = taps + (long)p * tstride;
            float acc0 = 0.0f, acc1 = 0.0f;
            for (int i = 0; i < a.K; ++i) {
                const float t = k[i];
                acc0 = fmaf(t, xs0[at + i], acc0);
                acc1 = fmaf(t, xs1[at + i], acc1);
            }
            acc0 = clamp1(acc0), acc1 = clamp1(acc1);
            out0[r] = acc0, out1[r] = acc1;
            const uint32_t m0 = __float_as_uint(acc0) & 0x7fffffffu, m1 = __float_as_uint(acc1) & 0x7fffffffu;
            peak = max(peak, max(m0, m1));
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) peak = max(peak, (uint32_t)__shfl_xor((int)peak, off, 64));
    if ((tid & 63) == 0) wave_peak[tid >> 6] = peak;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < AUDIO_IN_THREADS / 64; ++w) peak = max(peak, wave_peak[w]);
        if (peak) atomicMax(a.peak_bits, peak);
    }
}

AudioInRequest to_request(const ace355_audio_in_request* rq) {
    AudioInRequest r{};
    r.format = rq->format, r.channels = rq->channels, r.o = rq->o, r.n = rq->n, r.K = rq->K, r.width = rq->width, r.frames = rq->frames;
    return r;
}

}  // namespace
}  // namespace ace355

using namespace ace355;

extern "C" {

int ace355_audio_in_plan(const ace355_audio_in_request* rq, ace355_audio_in_plan_info* out) {
    ACE_CHECK(rq && out, "audio_in_plan: null argument");
    const AudioInPlan p = plan_audio_in(to_request(rq));
    if (p.refusal) {
        set_error(std::string("audio_in_plan: ") + p.refusal);
        return ACE355_ERR_INVALID;
    }
    out->out_frames = p.out_frames, out->grid = p.grid, out->tile = p.tile, out->threads = p.threads, out->span = p.span;
    out->table_in_lds = p.table_in_lds, out->lds_bytes = p.lds_bytes, out->passthrough = p.passthrough;
    return ACE355_OK;
}

int ace355_audio_in_run(const ace355_audio_in_request* rq, const void* payload_dev, int64_t payload_bytes, int64_t payload_offset,
                        const int32_t* first_dev, const float* taps_dev, float* out_dev, float* peak_dev, void* stream) {
    ACE_CHECK(rq && payload_dev && out_dev && peak_dev, "audio_in_run: null argument");
    const AudioInPlan p = plan_audio_in(to_request(rq));
    if (p.refusal) {
        set_error(std::string("audio_in_run: ") + p.refusal);
        return ACE355_ERR_INVALID;
    }
    ACE_CHECK(p.passthrough || (first_dev && taps_dev), "audio_in_run: a resampling request needs the tap table");
    ACE_CHECK((reinterpret_cast<uintptr_t>(payload_dev) & 3) == 0, "audio_in_run: the payload buffer must be 4-byte aligned (the payload inside it need not be)");
    const int64_t need = rq->frames * rq->channels * audio_in_sample_bytes(rq->format);
    ACE_CHECK(payload_offset >= 0 && payload_bytes >= 0 && payload_offset <= payload_bytes && need <= payload_bytes - payload_offset,
              "audio_in_run: the payload does not hold frames x channels samples at that offset");
    AudioInArgs a{};
    a.words = static_cast<const uint32_t*>(payload_dev), a.byte0 = payload_offset, a.first = first_dev, a.taps = taps_dev, a.out = out_dev;
    a.peak_bits = reinterpret_cast<uint32_t*>(peak_dev), a.frames = rq->frames, a.out_frames = p.out_frames, a.channels = rq->channels;
    a.o = rq->o, a.n = rq->n, a.K = rq->K, a.width = rq->width, a.tile = p.tile, a.span = p.span, a.table_in_lds = p.table_in_lds;
    hipStream_t s = (hipStream_t)stream;
    ACE_HIP(hipMemsetAsync(peak_dev, 0, sizeof(float), s));
    const dim3 grid((unsigned)p.grid), block(AUDIO_IN_THREADS);
    switch (rq->format) {
        case ACE355_PCM_U8: hipLaunchKernelGGL(audio_in_kernel<ACE355_PCM_U8>, grid, block, p.lds_bytes, s, a); break;
        case ACE355_PCM_S16: hipLaunchKernelGGL(audio_in_kernel<ACE355_PCM_S16>, grid, block, p.lds_bytes, s, a); break;
        case ACE355_PCM_S24: hipLaunchKernelGGL(audio_in_kernel<ACE355_PCM_S24>, grid, block, p.lds_bytes, s, a); break;
        case ACE355_PCM_S32: hipLaunchKernelGGL(audio_in_kernel<ACE355_PCM_S32>, grid, block, p.lds_bytes, s, a); break;
        default: hipLaunchKernelGGL(audio_in_kernel<ACE355_PCM_F32>, grid, block, p.lds_bytes, s, a); break;
    }
    ACE_LAUNCH_CHECK();
    return ACE355_OK;
}

}  // extern "C"
