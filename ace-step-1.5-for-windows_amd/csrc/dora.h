// dora.h - the DoRA (weight-decomposed) epilogue of the two merge kernels (lora.hip, lokr.hip; ace355_dit_set_adapters_dora).  Both
// kernels give a thread the same elements of a 64 x 128 tile: the 8-column group c8 = 8 (tid & 15) of the rows (tid >> 4) + 16 i,
// i < 4, as the fp32 values V = float(W0) + sum_j dW_j they would round.  Pass 1 reduces V^2 in fp64 along the tile's columns (axis
// "out") or rows (axis "in") and writes one partial per (row, column tile) resp. (row tile, column); dora_factor_kernel (dora.hip)
// adds the partials in tile order and forms f; pass 2 forms V again and writes bf16_rne(V * f).  No atomics: every order is fixed.
#pragma once
#include "common.h"

namespace ace355 {

// pass 1 needs DORA_LDS_DOUBLES doubles of LDS (the four waves' column sums of axis "in")
constexpr int DORA_LDS_DOUBLES = 4 * 128;

template <int PASS>
__device__ __forceinline__ void dora_epilogue(const LoraTargetDev& t, const DoraDev& d, int n0, int c0, int tid, const float (&v)[4][8],
                                              const bool (&live)[4], const long (&off)[4], double* sQ) {
    const int c8 = (tid & 15) * 8, rb = tid >> 4;
    if constexpr (PASS == 1) {
        if (!d.per_input) {
            // a row of the tile = the 16 lanes that share tid >> 4: 8 squares in column order per lane, then a butterfly over the lanes
            // (every lane of a wave takes part: a group outside the weight adds zeros)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                double q = 0.0;
                if (live[i]) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) q += (double)v[i][k] * (double)v[i][k];
                }
                q += __shfl_xor(q, 1);
                q += __shfl_xor(q, 2);
                q += __shfl_xor(q, 4);
                q += __shfl_xor(q, 8);
                const int n = n0 + rb + 16 * i;
                if ((tid & 15) == 0 && n < t.rows) d.part[(long)(c0 / LORA_TILE_COLS) * t.rows + n] = q;
            }
        } else {
            // a column of the tile: a thread's 4 rows in row order, the 4 lanes of a wave that share the column group (a butterfly),
            // then the 4 waves in wave order through LDS
            const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                double q = 0.0;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (live[i]) q += (double)v[i][k] * (double)v[i][k];
                q += __shfl_xor(q, 16);
                q += __shfl_xor(q, 32);
                if (lane < 16) sQ[wave * 128 + c8 + k] = q;
            }
            __syncthreads();
            const int c = c0 + tid;
            if (tid < 128 && c < t.cols)
                d.part[(long)(n0 / LORA_TILE_ROWS) * t.cols + c] = ((sQ[tid] + sQ[128 + tid]) + sQ[256 + tid]) + sQ[384 + tid];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (!live[i]) continue;
            float f[8];
            if (!d.per_input) {
                const float fr = d.f[n0 + rb + 16 * i];
#pragma unroll
                for (int k = 0; k < 8; ++k) f[k] = fr;
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) f[k] = d.f[c0 + c8 + k];
            }
            uint4 o;
            o.x = pack_bf2(v[i][0] * f[0], v[i][1] * f[1]);
            o.y = pack_bf2(v[i][2] * f[2], v[i][3] * f[3]);
            o.z = pack_bf2(v[i][4] * f[4], v[i][5] * f[5]);
            o.w = pack_bf2(v[i][6] * f[6], v[i][7] * f[7]);
            *reinterpret_cast<uint4*>(t.dst + off[i]) = o;
        }
    }
}

}  // namespace ace355
