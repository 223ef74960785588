// dora.hip - DoRA (weight-decomposed LoRA / LoKr) merged into the packed DiT weights (ace355_dit_set_adapters_dora): the step between
// the two passes of the merge kernels (dora.h).  Per row (axis "out") or column (axis "in") of a target it adds the fp64 partial sums
// of squares of V = float(W0) + sum_j dW_j in tile order and forms, in fp64,
//     n = sqrt(sum),   f = 1 + m (g / (n + eps) - 1)   (f = 1 where n + eps == 0),
// rounded to fp32 once.  Pass 2 then writes bf16_rne(V * f).
#include "../../include/ace355.h"
#include "common.h"

namespace ace355 {

namespace {

// grid (chunks of 256 indices, targets)
__global__ __launch_bounds__(256) void dora_factor_kernel(const DoraDev* __restrict__ dora) {
    const DoraDev d = dora[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.n) return;
    double sum = 0.0;
    for (int k = 0; k < d.ntiles; ++k) sum += d.part[(long)k * d.n + i];
    const double den = sqrt(sum) + (double)d.eps;
    const double f = den == 0.0 ? 1.0 : 1.0 + (double)d.m * ((double)d.g[i] / den - 1.0);
    d.f[i] = (float)f;
}

}  // namespace

int launch_dora_factors(const DoraDev* dora_dev, int n_targets, int chunks, hipStream_t s) {
    if (n_targets <= 0 || chunks <= 0) return 0;
    hipLaunchKernelGGL(dora_factor_kernel, dim3(chunks, n_targets), dim3(256), 0, s, dora_dev);
    ACE_LAUNCH_CHECK();
    return 0;
}

}  // namespace ace355
