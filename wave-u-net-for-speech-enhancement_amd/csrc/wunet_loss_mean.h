// The three element-wise mean losses (include/wunet_hip.h: wunet_loss_forward / wunet_loss_backward): the batch as one flat array.
//   loss_partial_kernel   one pass over the pair: a block's sum of terms, in double
//   loss_final_kernel     the blocks' sums in a fixed order -> the mean, rounded to float once
//   loss_bwd_kernel       grad_enh[i] = gscale[0] * dterm(enh - clean) / n, streaming
#pragma once
#include "wunet_reduce.h"

// ---------------------------------------------------------------------------- losses
// loss(clean, enhanced) of trainer/trainer.py:36; kind 0 = MSELoss, 1 = L1Loss (model/loss.py:3-7),
// 2 = SmoothL1Loss(beta=1).  mean reduction.
__device__ __forceinline__ float loss_term(int kind, float d)
{
    if (kind == 0) return d * d;
    const float ad = fabsf(d);
    if (kind == 1) return ad;
    return ad < 1.0f ? 0.5f * d * d : ad - 0.5f;
}
__device__ __forceinline__ float loss_dterm(int kind, float d)   // derivative w.r.t. d = enhanced - clean
{
    if (kind == 0) return 2.0f * d;
    const float sg = (d > 0.0f ? 1.0f : 0.0f) - (d < 0.0f ? 1.0f : 0.0f);
    if (kind == 1) return sg;
    return fabsf(d) < 1.0f ? d : sg;
}

static __global__ __launch_bounds__(WUNET_THREADS) void loss_partial_kernel(int kind, const float* clean, const float* enh, size_t n, double* part)
{
    __shared__ double red[WUNET_WAVES];
    double s[1] = {0.0};
    // four trips' loads in flight (a thread's 16 trips at batch 64 x 16384 were 16 dependent memory round trips: 10.4 us for 8 MB); the terms are
    // added in the one-trip loop's order - the same bits
    const size_t stride = (size_t)gridDim.x * WUNET_THREADS;
    size_t i = (size_t)blockIdx.x * WUNET_THREADS + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {
        float e[4], c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { e[u] = enh[i + u * stride]; c[u] = clean[i + u * stride]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) s[0] += (double)loss_term(kind, e[u] - c[u]);
    }
    for (; i < n; i += stride) s[0] += (double)loss_term(kind, enh[i] - clean[i]);
    block_sum<1>(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}

static __global__ __launch_bounds__(WUNET_THREADS) void loss_final_kernel(const double* part, int rows, size_t n, float* loss)
{
    __shared__ double red[WUNET_WAVES];
    double s[1] = {0.0};
    for (int r = threadIdx.x; r < rows; r += WUNET_THREADS) s[0] += part[r];
    block_sum<1>(s, red);
    if (threadIdx.x == 0) *loss = (float)(s[0] / (double)n);
}

// grad_enh[i] = gscale[0] * dterm(enh - clean) / n
static __global__ __launch_bounds__(WUNET_THREADS) void loss_bwd_kernel(int kind, const float* clean, const float* enh, const float* gscale, size_t n, float* genh)
{
    const float sc = gscale[0] / (float)n;
    const size_t stride = (size_t)gridDim.x * WUNET_THREADS;
    size_t i = (size_t)blockIdx.x * WUNET_THREADS + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {             // (four trips' loads ahead of the first store)
        float e[4], c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { e[u] = enh[i + u * stride]; c[u] = clean[i + u * stride]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) genh[i + u * stride] = sc * loss_dterm(kind, e[u] - c[u]);
    }
    for (; i < n; i += stride) genh[i] = sc * loss_dterm(kind, enh[i] - clean[i]);
}
