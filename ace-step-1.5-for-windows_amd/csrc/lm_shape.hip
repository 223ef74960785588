// lm_shape.hip - the logits stage of the 5 Hz LM's CFG loop behind ace355.h: what the reference does to
// the logits between its forward and its token selection (llm_inference.py:2482-2493) - the CFG combine, the codes-phase / COMPLETED /
// disabled branches of MetadataConstrainedLogitsProcessor.__call__ with _apply_temperature_scaling (constrained_logits_processor.py:
// 1583-1629, 1666-1695) and transformers' RepetitionPenaltyLogitsProcessor - as ONE elementwise launch, and the bitmap of seen ids the
// penalty reads.
//
// Every output element is a function of its own inputs alone, rounded to fp32 after every operation and never contracted into an fma
// (contraction is off for this file, by the pragma below and by build.py's FILE_FLAGS, and the operations are plain operators: the
// __f*_rn intrinsics are inlined from a header that allows contraction, so the pragma does not reach them), so it carries the bits of
// the reference's chain of separate torch kernels.  A row is cut by lm_plan.h's plan_lm_pick(V) like the selection that follows; the cut cannot change
// a bit.  No LDS, no scratch, no floating-point atomics; ace355_lm_seen_mark's integer atomicOr commutes.
//
// ace355_lm_shape_as is the same launch in the model's dtype: the reference's non-CFG loop (llm_inference.py:2369-2377) never upcasts,
// so on a bf16 model every one of its torch kernels rounds its result to bf16.  The kernel is templated on the dtype; the BF16
// instantiation rounds where torch rounds (bf16_rne below, an integer operation on the bit pattern), the F32 one is the code as it was.
#include <math.h>

#include <string>

#include "../../include/ace355.h"
#include "common.h"
#include "lm_plan.h"

#pragma clang fp contract(off)

using namespace ace355;

namespace {

struct ShapeArgs {
    const float *cond, *uncond;   // uncond == nullptr: no CFG
    float* out;                   // may be cond
    long cond_stride, uncond_stride, out_stride;
    const float* mask;            // [V] or nullptr
    const uint32_t* seen;         // [B][words] or nullptr
    int V, words, chunk;
    int eos_id, eos_mode;         // 0 none, 1 block, 2 force
    int has_temperature, use_penalty;
    float cfg_scale, temperature, penalty;
};

// 4 fp32 that are only 4-byte aligned: dense rows of an odd V start anywhere (the hardware takes a dword-aligned 16-byte access)
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// round-to-nearest-even of an fp32 value to bf16, kept in fp32: +-inf and +-0 stay, subnormals round like any value, a finite value
// past bf16's largest becomes inf, a NaN stays a (quiet) NaN
__device__ __forceinline__ float bf16_rne(float x) {
    uint32_t b = __float_as_uint(x);
    if ((b & 0x7fffffffu) > 0x7f800000u) return __uint_as_float((b & 0x80000000u) | 0x7fc00000u);
    b += 0x7fffu + ((b >> 16) & 1u);
    return __uint_as_float(b & 0xffff0000u);
}

template <int DT>
__device__ __forceinline__ float shape_one(const ShapeArgs& a, float c, float u, float m, uint32_t seen_word, int v) {
    if constexpr (DT == ACE355_DTYPE_BF16) {   // no CFG below fp32 (refused on the host): c -> bf16, then every result -> bf16
        float x = bf16_rne(c);
        if (a.mask) x = bf16_rne(x + bf16_rne(m));
        if (a.eos_mode == 1 && v == a.eos_id) x = -INFINITY;
        if (a.eos_mode == 2 && v != a.eos_id) x = -INFINITY;
        if (a.has_temperature) x = bf16_rne(x / a.temperature);
        if (a.use_penalty && ((seen_word >> (v & 31)) & 1u)) x = x < 0.f ? bf16_rne(x * a.penalty) : bf16_rne(x / a.penalty);
        return x;
    }
    float x = c;
    if (a.uncond) {
        const float d = c - u;
        const float sd = a.cfg_scale * d;
        x = u + sd;
    }
    if (a.mask) x = x + m;
    if (a.eos_mode == 1 && v == a.eos_id) x = -INFINITY;
    if (a.eos_mode == 2 && v != a.eos_id) x = -INFINITY;
    if (a.has_temperature) x = x / a.temperature;
    if (a.use_penalty && ((seen_word >> (v & 31)) & 1u)) x = x < 0.f ? x * a.penalty : x / a.penalty;
    return x;
}

template <int DT>
__device__ __forceinline__ void shape_scalar(const ShapeArgs& a, const float* c, const float* u, float* o, const uint32_t* seen, int v) {
    o[v] = shape_one<DT>(a, c[v], u ? u[v] : 0.f, a.mask ? a.mask[v] : 0.f, seen ? seen[v >> 5] : 0u, v);
}

// grid (chunks, B).  Row b: the ids before `out`'s first 16-byte boundary (head, < 4) and those after the last whole group of four
// (tail, < 4) go one by one; the groups in between, each owned by the chunk that holds its first id, are 16-byte stores and 16-byte
// loads.  Every id is written exactly once, by the thread that read it, so `out` may be `cond`.
template <int DT>
__global__ __launch_bounds__(256) void lm_shape_kernel(ShapeArgs a) {
    const int b = blockIdx.y, V = a.V;
    const float* c = a.cond + (long)b * a.cond_stride;
    const float* u = a.uncond ? a.uncond + (long)b * a.uncond_stride : nullptr;
    float* o = a.out + (long)b * a.out_stride;
    const uint32_t* seen = a.seen ? a.seen + (long)b * a.words : nullptr;
    const int head = min(V, (int)((4 - ((reinterpret_cast<uintptr_t>(o) >> 2) & 3)) & 3));
    const int groups = (V - head) >> 2;
    const int lo = blockIdx.x * a.chunk, hi = min(V, lo + a.chunk);

    if (blockIdx.x == 0 && (int)threadIdx.x < head) shape_scalar<DT>(a, c, u, o, seen, threadIdx.x);
    const int tail0 = head + 4 * groups;
    if (blockIdx.x == gridDim.x - 1 && (int)threadIdx.x < V - tail0) shape_scalar<DT>(a, c, u, o, seen, tail0 + threadIdx.x);

    // groups g with lo <= head + 4 g < hi
    const int g_lo = lo <= head ? 0 : (lo - head + 3) >> 2;
    const int g_hi = min(groups, hi <= head ? 0 : (hi - head + 3) >> 2);
    for (int g = g_lo + threadIdx.x; g < g_hi; g += 256) {
        const int v0 = head + 4 * g;
        const f32x4_a4 cv = *reinterpret_cast<const f32x4_a4*>(c + v0);
        f32x4_a4 uv = {0.f, 0.f, 0.f, 0.f}, mv = {0.f, 0.f, 0.f, 0.f};
        if (u) uv = *reinterpret_cast<const f32x4_a4*>(u + v0);
        if (a.mask) mv = *reinterpret_cast<const f32x4_a4*>(a.mask + v0);
        uint32_t w0 = 0u, w1 = 0u;   // v0 .. v0 + 3 touch at most two words of the bitmap
        if (seen) { w0 = seen[v0 >> 5]; w1 = seen[(v0 + 3) >> 5]; }
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = shape_one<DT>(a, cv[e], uv[e], mv[e], ((v0 + e) >> 5) == (v0 >> 5) ? w0 : w1, v0 + e);
        *reinterpret_cast<f32x4*>(o + v0) = r;
    }
}

// ids [B, T] -> bit v & 31 of word v >> 5 of row b, for every id in [0, V); one thread per id
__global__ __launch_bounds__(256) void lm_seen_mark_kernel(const int64_t* __restrict__ ids, long row_stride, int T, int V, int words,
                                                           uint32_t* __restrict__ seen) {
    const int t = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (t >= T) return;
    const int64_t v = ids[(long)b * row_stride + t];
    if (v < 0 || v >= V) return;
    atomicOr(seen + (long)b * words + (v >> 5), 1u << (v & 31));
}

int refuse(const char* who, const std::string& msg) {
    set_error(std::string(who) + ": " + msg);
    return ACE355_ERR_INVALID;
}

// the checks and the launch behind ace355_lm_shape (dtype F32) and ace355_lm_shape_as
int launch_shape(const char* who, const float* cond_dev, int64_t cond_stride, const float* uncond_dev, int64_t uncond_stride,
                 float* out_dev, int64_t out_stride, int B, int V, const ace355_lm_shape_params* p, int dtype, void* stream) {
    if (dtype != ACE355_DTYPE_F32 && dtype != ACE355_DTYPE_BF16) return refuse(who, "dtype must be ACE355_DTYPE_F32 or ACE355_DTYPE_BF16");
    if (uncond_dev && dtype != ACE355_DTYPE_F32) return refuse(who, "uncond (the CFG combine) is taken in fp32 only");
    if (B < 1 || B > ACE355_LM_MAX_SEQS) return refuse(who, "B must be 1 .. " + std::to_string(ACE355_LM_MAX_SEQS));
    if (V < 1 || V > LM_PICK_MAX_V) return refuse(who, "V must be 1 .. " + std::to_string(LM_PICK_MAX_V));
    if (!cond_dev || !out_dev || !p) return refuse(who, "cond, out and params must not be null");
    if (cond_stride < V || out_stride < V || (uncond_dev && uncond_stride < V)) return refuse(who, "a row stride is smaller than V");
    if (p->eos_mode < 0 || p->eos_mode > 2) return refuse(who, "eos_mode must be 0 (none), 1 (block) or 2 (force)");
    if (p->eos_mode != 0 && (p->eos_id < 0 || p->eos_id >= V)) return refuse(who, "eos_id outside [0, V)");
    if (!(p->penalty > 0.f) || isinf(p->penalty)) return refuse(who, "penalty must be finite and > 0");
    if (p->penalty != 1.f && !p->seen) return refuse(who, "seen is required when penalty != 1");
    if (uncond_dev && p->cfg_scale != p->cfg_scale) return refuse(who, "cfg_scale must not be NaN");
    if (p->has_temperature && !(p->temperature > 0.f)) return refuse(who, "temperature must be > 0 (map T <= 0 to 1e-6 as the reference does)");

    const LmPickPlan plan = plan_lm_pick(V);
    ShapeArgs a{};
    a.cond = cond_dev; a.uncond = uncond_dev; a.out = out_dev;
    a.cond_stride = cond_stride; a.uncond_stride = uncond_stride; a.out_stride = out_stride;
    a.mask = p->mask;
    a.use_penalty = p->penalty != 1.f;
    a.seen = a.use_penalty ? p->seen : nullptr;
    a.V = V; a.words = (V + 31) / 32; a.chunk = plan.chunk;
    a.eos_id = p->eos_id; a.eos_mode = p->eos_mode;
    a.has_temperature = p->has_temperature != 0;
    a.cfg_scale = p->cfg_scale; a.temperature = p->temperature; a.penalty = p->penalty;
    if (dtype == ACE355_DTYPE_BF16)
        hipLaunchKernelGGL(lm_shape_kernel<ACE355_DTYPE_BF16>, dim3(plan.chunks, B), dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(lm_shape_kernel<ACE355_DTYPE_F32>, dim3(plan.chunks, B), dim3(256), 0, (hipStream_t)stream, a);
    ACE_LAUNCH_CHECK();
    return ACE355_OK;
}

}  // namespace

extern "C" {

int ace355_lm_shape(const float* cond_dev, int64_t cond_stride, const float* uncond_dev, int64_t uncond_stride, float* out_dev,
                    int64_t out_stride, int B, int V, const ace355_lm_shape_params* p, void* stream) {
    return launch_shape("lm_shape", cond_dev, cond_stride, uncond_dev, uncond_stride, out_dev, out_stride, B, V, p, ACE355_DTYPE_F32, stream);
}

int ace355_lm_shape_as(const float* cond_dev, int64_t cond_stride, const float* uncond_dev, int64_t uncond_stride, float* out_dev,
                       int64_t out_stride, int B, int V, const ace355_lm_shape_params* p, int dtype, void* stream) {
    return launch_shape("lm_shape_as", cond_dev, cond_stride, uncond_dev, uncond_stride, out_dev, out_stride, B, V, p, dtype, stream);
}

int ace355_lm_seen_mark(const int64_t* ids_dev, int64_t row_stride, int B, int T, int V, uint32_t* seen_dev, void* stream) {
    static const char* who = "lm_seen_mark";
    if (B < 1 || B > ACE355_LM_MAX_SEQS) return refuse(who, "B must be 1 .. " + std::to_string(ACE355_LM_MAX_SEQS));
    if (V < 1 || V > LM_PICK_MAX_V) return refuse(who, "V must be 1 .. " + std::to_string(LM_PICK_MAX_V));
    if (T < 1 || T > ACE355_LM_MAX_POSITIONS) return refuse(who, "T must be 1 .. " + std::to_string(ACE355_LM_MAX_POSITIONS));
    if (row_stride < T) return refuse(who, "row_stride is smaller than T");
    if (!ids_dev || !seen_dev) return refuse(who, "ids and seen must not be null");
    hipLaunchKernelGGL(lm_seen_mark_kernel, dim3((T + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, ids_dev, (long)row_stride, T, V,
                       (V + 31) / 32, seen_dev);
    ACE_LAUNCH_CHECK();
    return ACE355_OK;
}

}  // extern "C"
