// lm_score.hip - teacher-forced scoring on the 5 Hz LM's head behind ace355.h: for R rows of final-norm
// activations and one target id each, the target's log-probability and its 0-based rank among the V logits of its row - what the
// reference's quality score (acestep/core/scoring/lm_score.py) takes from a [T, V] logits tensor on the host - without the logits ever
// leaving the workgroup that made them.
//
// Three launches.  (1) The pre-pass gives every row its counting threshold z_r = x_r . W[t_r].  (2) The fused head: a workgroup takes
// 64 rows and one chunk of ids (lm_plan.h: plan_lm_score), forms the logits of 256 ids at a time with 32x32x16 MFMAs, and folds them
// into a running maximum, a sum of exponentials, the two counts of the rank and the target's own logit; one partial per (row, chunk)
// leaves the workgroup.  (3) The merge combines a row's partials.  There is no atomic: a lane folds its ids in ascending order, a
// workgroup its 8 lane groups in a fixed order, the merge the chunks by a fixed lane assignment, so the same call gives the same bits;
// and because the cut of the vocabulary is a function of V alone and a row's arithmetic does not depend on its place in a tile, a row's
// bits do not depend on the rows beside it.
//
// A logit is summed in two levels: the MFMAs of FLUSH_SLICES K slices (256 k) chain into one accumulator, which is then added to the
// logit's total in plain fp32 and cleared.  One chain over D = 2048 is 128 dependent fp32 accumulations, and its error showed in the
// last bits of the log-probability; 16-step chains plus 8 adds stay at what a host fp32 matrix product makes of the same inputs.
//
// The pre-pass runs the SAME two-level chain as the head (k ascending in steps of 16), so z_r is bit for bit the
// head's own logit of the target, and an id whose W row equals the target's compares equal to z_r: ties are then ordered by id, as
// lm_sample.hip orders them.
#include <math.h>

#include <string>

#include "../../include/ace355.h"
#include "common.h"
#include "lm_plan.h"

using namespace ace355;

namespace {

constexpr int TM = LM_SCORE_TILE_ROWS, TN = LM_SCORE_STEP_IDS, BK = LM_SCORE_K_SLICE;
constexpr int LDK = BK + 8;   // LDS row pitch in bf16: 144 bytes = 36 banks, so the 16 lanes of a ds_read_b128 group hit 16 distinct bank quads
constexpr int FLUSH_SLICES = 4;   // K slices whose MFMAs chain into one accumulator before it is added to the total
constexpr float LOG2E = 1.4426950408889634f;
static_assert(TM == 64 && TN == 256 && BK == 64, "the thread maps below are written for a 64 x 256 x 64 step and 4 waves");

struct ScorePart {
    float m, s;    // max of the chunk's logits of this row, sum of exp(logit - m); m = -inf, s = 0 never happens (a chunk holds an id < V)
    int gt, eq;    // ids != t with logit > z; with logit == z and id < t
    float t;       // the target's logit, valid when has != 0 (the one chunk that holds t)
    int has;
    int pad[2];
};
static_assert(sizeof(ScorePart) == LM_SCORE_PART_BYTES, "lm_plan.h sizes the workspace");

__device__ __forceinline__ int clamp_id(int t, int V) { return t < 0 ? 0 : (t >= V ? V - 1 : t); }

// ------------------------------------------------------------------------------------------------ (1) thresholds
// One wave per row: every A row of the MFMA is W[t_r], every B column is x_r, so all 32 x 32 results are z_r; lane 0 register 0 is written.
__global__ __launch_bounds__(64) void score_z_kernel(const bf16_t* __restrict__ x, long x_stride, const int* __restrict__ row_index,
                                                     const bf16_t* __restrict__ W, const int* __restrict__ targets, int V, int D,
                                                     float* __restrict__ z) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const long xr = row_index ? row_index[r] : r;
    const bf16_t* wp = W + (long)clamp_id(targets[r], V) * D + (lane >> 5) * 8;
    const bf16_t* xp = x + xr * x_stride + (lane >> 5) * 8;
    float tot = 0.f;
    for (int g0 = 0; g0 < D; g0 += FLUSH_SLICES * BK) {
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        const int g1 = min(D, g0 + FLUSH_SLICES * BK);
        for (int k0 = g0; k0 < g1; k0 += 16) acc = mfma32(as_bf16x8(ldg16(wp + k0)), as_bf16x8(ldg16(xp + k0)), acc);
        tot += acc[0];
    }
    if (lane == 0) z[r] = tot;
}

// ------------------------------------------------------------------------------------------------ (2) the fused head
// 256 threads = 4 waves.  Per column step the workgroup forms logits[64 rows][256 ids]: W is the A operand (i = id), x the B operand
// (j = row), so a lane holds ONE row (j = lane & 31, per row block) and 16 ids per accumulator, and every per-row fold is in-lane.
// Wave w owns ids [64 w, 64 w + 64) of the step (2 id blocks) x both row blocks: 4 accumulators.  K slices of both operands are staged
// through LDS (global -> registers one slice ahead -> LDS), K-contiguous in both.
struct ScoreArgs {
    const bf16_t* x; long x_stride; const int* row_index;
    const bf16_t* W; const int* targets; const float* z;
    int R, V, D, chunk;
    ScorePart* parts; int chunks;
};

// (128 accumulator registers + the staging registers fit 256 VGPRs without scratch: two workgroups per CU, so one's fold and barriers
// hide under the other's K loop)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void score_head_kernel(ScoreArgs a) {
    __shared__ __attribute__((aligned(16))) bf16_t sx[TM * LDK];
    __shared__ __attribute__((aligned(16))) bf16_t sw[TN * LDK];
    __shared__ float red_m[8][TM], red_s[8][TM], red_t[8][TM];
    __shared__ int red_gt[8][TM], red_eq[8][TM], red_has[8][TM];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
    const int row0 = blockIdx.x * TM, c = blockIdx.y;
    const int id_lo = c * a.chunk;
    const int nks = a.D / BK;

    // staging map: piece p = tid + 256 i is 16 bytes: tile row p >> 3, k piece p & 7
    const int s_row = tid >> 3, s_kp = tid & 7;
    const bf16_t* xg[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = min(row0 + s_row + 32 * i, a.R - 1);   // rows beyond R repeat the last one; their results are dropped
        const long xr = a.row_index ? a.row_index[r] : r;
        xg[i] = a.x + xr * a.x_stride + s_kp * 8;
    }

    // this lane's two rows (row block rb): target, threshold and the running fold
    int tgt[2];
    float zz[2], m[2], s[2], tv[2];
    int gt[2], eq[2], has[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const int r = min(row0 + rb * 32 + col, a.R - 1);
        tgt[rb] = a.targets[r];
        zz[rb] = a.z[r];
        m[rb] = -INFINITY; s[rb] = 0.f; tv[rb] = 0.f;
        gt[rb] = 0; eq[rb] = 0; has[rb] = 0;
    }

    for (int id0 = id_lo; id0 < id_lo + a.chunk && id0 < a.V; id0 += TN) {
        const bf16_t* wg[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) wg[i] = a.W + (long)min(id0 + s_row + 32 * i, a.V - 1) * a.D + s_kp * 8;   // no row of W at or beyond V is read

        f32x16 acc[2][2], tot[2][2];   // [id block][row block]: the running chain and the logits' totals
#pragma unroll
        for (int ab = 0; ab < 2; ++ab)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int i = 0; i < 16; ++i) { acc[ab][rb][i] = 0.f; tot[ab][rb][i] = 0.f; }

        uint4 px[2], pw[8];
#pragma unroll
        for (int i = 0; i < 2; ++i) px[i] = ldg16(xg[i]);
#pragma unroll
        for (int i = 0; i < 8; ++i) pw[i] = ldg16(wg[i]);

        for (int ks = 0; ks < nks; ++ks) {
            __syncthreads();   // the previous slice (or the previous step's fold) has been read
#pragma unroll
            for (int i = 0; i < 2; ++i) *reinterpret_cast<uint4*>(&sx[(s_row + 32 * i) * LDK + s_kp * 8]) = px[i];
#pragma unroll
            for (int i = 0; i < 8; ++i) *reinterpret_cast<uint4*>(&sw[(s_row + 32 * i) * LDK + s_kp * 8]) = pw[i];
            __syncthreads();
            if (ks + 1 < nks) {
                const int k1 = (ks + 1) * BK;
#pragma unroll
                for (int i = 0; i < 2; ++i) px[i] = ldg16(xg[i] + k1);
#pragma unroll
                for (int i = 0; i < 8; ++i) pw[i] = ldg16(wg[i] + k1);
            }
#pragma unroll
            for (int kk = 0; kk < BK / 16; ++kk) {
                const int ko = kk * 16 + half * 8;
                const bf16x8 a0 = as_bf16x8(*reinterpret_cast<const uint4*>(&sw[(wave * 64 + col) * LDK + ko]));
                const bf16x8 a1 = as_bf16x8(*reinterpret_cast<const uint4*>(&sw[(wave * 64 + 32 + col) * LDK + ko]));
                const bf16x8 b0 = as_bf16x8(*reinterpret_cast<const uint4*>(&sx[col * LDK + ko]));
                const bf16x8 b1 = as_bf16x8(*reinterpret_cast<const uint4*>(&sx[(32 + col) * LDK + ko]));
                // (consecutive MFMAs alternate their A registers)
                acc[0][0] = mfma32(a0, b0, acc[0][0]);
                acc[1][0] = mfma32(a1, b0, acc[1][0]);
                acc[0][1] = mfma32(a0, b1, acc[0][1]);
                acc[1][1] = mfma32(a1, b1, acc[1][1]);
            }
            if ((ks + 1) % FLUSH_SLICES == 0 || ks + 1 == nks) {
#pragma unroll
                for (int ab = 0; ab < 2; ++ab)
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                        for (int i = 0; i < 16; ++i) { tot[ab][rb][i] += acc[ab][rb][i]; acc[ab][rb][i] = 0.f; }
            }
        }

        // fold this step's 2 x 16 logits of each of the lane's rows, ids ascending
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            float mx = m[rb];
#pragma unroll
            for (int ab = 0; ab < 2; ++ab)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int id = id0 + wave * 64 + ab * 32 + mfma_row(r, lane);
                    if (id < a.V) mx = fmaxf(mx, tot[ab][rb][r]);
                }
            if (mx > -INFINITY) {   // (a lane whose ids are all >= V so far has nothing to fold)
                float sum = s[rb] * __builtin_amdgcn_exp2f((m[rb] - mx) * LOG2E);   // m = -inf: exp2(-inf) = 0 and s = 0
#pragma unroll
                for (int ab = 0; ab < 2; ++ab)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int id = id0 + wave * 64 + ab * 32 + mfma_row(r, lane);
                        const float v = tot[ab][rb][r];
                        if (id < a.V) {
                            sum += __builtin_amdgcn_exp2f((v - mx) * LOG2E);
                            if (id == tgt[rb]) { tv[rb] = v; has[rb] = 1; }
                            else {
                                gt[rb] += v > zz[rb] ? 1 : 0;
                                eq[rb] += (v == zz[rb] && id < tgt[rb]) ? 1 : 0;
                            }
                        }
                    }
                s[rb] = sum;
                m[rb] = mx;
            }
        }
    }

    // the 8 lane groups (wave, half) of a row, in group order
    const int g = wave * 2 + half;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const int tr = rb * 32 + col;
        red_m[g][tr] = m[rb]; red_s[g][tr] = s[rb]; red_t[g][tr] = tv[rb];
        red_gt[g][tr] = gt[rb]; red_eq[g][tr] = eq[rb]; red_has[g][tr] = has[rb];
    }
    __syncthreads();
    if (tid < TM && row0 + tid < a.R) {
        float M = -INFINITY;
#pragma unroll
        for (int i = 0; i < 8; ++i) M = fmaxf(M, red_m[i][tid]);
        ScorePart p{};
        p.m = M;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (red_m[i][tid] > -INFINITY) p.s += red_s[i][tid] * __builtin_amdgcn_exp2f((red_m[i][tid] - M) * LOG2E);
            p.gt += red_gt[i][tid];
            p.eq += red_eq[i][tid];
            if (red_has[i][tid]) { p.t = red_t[i][tid]; p.has = 1; }
        }
        a.parts[(long)(row0 + tid) * a.chunks + c] = p;
    }
}

// ------------------------------------------------------------------------------------------------ (3) merge
// One wave per row.  Lane l takes chunks l, l + 64, ... in ascending order, then the lanes are added by wave_sum's fixed butterfly; the
// exponentials, the sum and the logarithm are fp64, so what is left of the order is far below the fp32 result's last bit.  The
// numerator is the head's own logit of the target, not z_r.  A target outside [0, V) is in no chunk: log-prob NaN, rank -1.
__global__ __launch_bounds__(64) void score_merge_kernel(const ScorePart* __restrict__ parts, int chunks, float* __restrict__ logprob,
                                                         int* __restrict__ rank) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const ScorePart* p = parts + (long)r * chunks;
    float M = -INFINITY;
    for (int c = lane; c < chunks; c += 64) M = fmaxf(M, p[c].m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
    double S = 0.0, T = 0.0;
    int cnt = 0, has = 0;
    for (int c = lane; c < chunks; c += 64) {
        const ScorePart q = p[c];
        if (q.m > -INFINITY) S += (double)q.s * exp((double)q.m - (double)M);
        cnt += q.gt + q.eq;
        if (q.has) { T += (double)q.t; has += 1; }   // exactly one chunk holds the target
    }
    S = wave_sum_d(S);
    T = wave_sum_d(T);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o, 64); has += __shfl_xor(has, o, 64); }
    if (lane == 0) {
        if (has == 1 && S > 0.0) {
            const double lp = T - ((double)M + log(S));
            logprob[r] = lp < 0.0 ? (float)lp : 0.f;
            rank[r] = cnt;
        } else {
            logprob[r] = __uint_as_float(0x7FC00000u);
            rank[r] = -1;
        }
    }
}

int refuse(const std::string& msg) {
    set_error("lm_score_rows: " + msg);
    return ACE355_ERR_INVALID;
}

}  // namespace

extern "C" {

size_t ace355_lm_score_workspace_bytes(int R, int V) { return (size_t)lm_score_workspace_bytes(R, V); }

int ace355_lm_score_plan(int R, int V, int D, int32_t* tile_rows_out, int32_t* chunk_out, int32_t* chunks_out, int32_t* grid_x_out,
                         int32_t* grid_y_out) {
    const LmScorePlan p = plan_lm_score(R, V, D);
    ACE_CHECK(tile_rows_out && chunk_out && chunks_out && grid_x_out && grid_y_out, "lm_score_plan: null argument");
    ACE_CHECK(p.chunks > 0, "lm_score_plan: R must be 1 .. 65536, V 1 .. 1048576, D a multiple of 64 up to 16384");
    *tile_rows_out = p.tile_rows;
    *chunk_out = p.chunk;
    *chunks_out = p.chunks;
    *grid_x_out = p.grid_x;
    *grid_y_out = p.grid_y;
    return ACE355_OK;
}

int ace355_lm_score_rows(const void* x_dev, int64_t x_row_stride, const int32_t* row_index_dev, const void* W_dev,
                         const int32_t* targets_dev, int R, int V, int D, float* logprob_dev, int32_t* rank_dev, void* workspace_dev,
                         size_t workspace_bytes, void* stream) {
    if (R < 1 || R > LM_SCORE_MAX_ROWS) return refuse("R must be 1 .. " + std::to_string(LM_SCORE_MAX_ROWS));
    if (V < 1 || V > LM_SCORE_MAX_V) return refuse("V must be 1 .. " + std::to_string(LM_SCORE_MAX_V));
    if (D < 1 || D > LM_SCORE_MAX_D || D % LM_SCORE_K_SLICE != 0)
        return refuse("D must be a multiple of " + std::to_string(LM_SCORE_K_SLICE) + " up to " + std::to_string(LM_SCORE_MAX_D));
    if (x_row_stride < D || x_row_stride % 8 != 0) return refuse("x_row_stride must be a multiple of 8 and at least D");
    if (!x_dev || !W_dev || !targets_dev || !logprob_dev || !rank_dev || !workspace_dev)
        return refuse("x, W, targets, logprob, rank and workspace must not be null");
    if (((uintptr_t)x_dev | (uintptr_t)W_dev | (uintptr_t)workspace_dev) & 15) return refuse("x, W and workspace must be 16-byte aligned");
    const LmScorePlan plan = plan_lm_score(R, V, D);
    const size_t need = (size_t)lm_score_workspace_bytes(R, V);
    if (plan.chunks == 0 || need == 0) return refuse("no plan for this request");
    if (workspace_bytes < need)
        return refuse("workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(need) + " needed");

    hipStream_t s = (hipStream_t)stream;
    float* z = (float*)workspace_dev;
    ScorePart* parts = (ScorePart*)((char*)workspace_dev + lm_score_align256((unsigned long long)R * 4));
    const bf16_t* x = (const bf16_t*)x_dev;
    const bf16_t* W = (const bf16_t*)W_dev;
    hipLaunchKernelGGL(score_z_kernel, dim3(R), dim3(64), 0, s, x, (long)x_row_stride, row_index_dev, W, targets_dev, V, D, z);
    ACE_LAUNCH_CHECK();
    const ScoreArgs a{x, (long)x_row_stride, row_index_dev, W, targets_dev, z, R, V, D, plan.chunk, parts, plan.chunks};
    hipLaunchKernelGGL(score_head_kernel, dim3(plan.grid_x, plan.grid_y), dim3(256), 0, s, a);
    ACE_LAUNCH_CHECK();
    hipLaunchKernelGGL(score_merge_kernel, dim3(R), dim3(64), 0, s, parts, plan.chunks, logprob_dev, rank_dev);
    ACE_LAUNCH_CHECK();
    return ACE355_OK;
}

}  // extern "C"
