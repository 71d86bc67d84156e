// The fused optimiser step (include/wunet_hip.h: wunet_adam_step, wunet_adam_step_ex).
//   grad_sqnorm_partial_kernel   the squared global norm of the scaled gradients, one double per block (gradient clipping only)
//   adam_hyper_kernel            the step's scalars into the hyper buffer: step counter, bias corrections, clip factor, decay
//   adam_kernel                  the update of up to WUNET_ADAM_MAX tensors per launch
// torch.optim.Adam(lr, betas, eps=1e-8, weight_decay=0, amsgrad=False) as the reference builds it (train.py:31-35), and on request
// gradient clipping by global norm (torch.nn.utils.clip_grad_norm_), decoupled weight decay (torch.optim.AdamW) and an lr read from
// device memory: per-step scalars that live in the hyper buffer, so a captured step replays unchanged under an lr schedule.
#pragma once
#include "wunet_reduce.h"

#define WUNET_ADAM_MAX 64
struct AdamTable {
    float* p[WUNET_ADAM_MAX];
    const float* g[WUNET_ADAM_MAX];
    float* m[WUNET_ADAM_MAX];
    float* v[WUNET_ADAM_MAX];
    unsigned n[WUNET_ADAM_MAX];
};

// Slots of the hyper buffer.  wunet_adam_step's buffer has the first two only; wunet_adam_step_ex's has WUNET_ADAM_HYPER_FLOATS
// (include/wunet_hip.h) - the kernels below touch the optional slots (2 and up) only when told that they exist.
#define WUNET_HYPER_STEP_SIZE 0
#define WUNET_HYPER_BC2_SQRT 1
#define WUNET_HYPER_CLIP 2        // min(1, max_norm / (norm + 1e-6)); 1 when clipping is off
#define WUNET_HYPER_NORM 3        // the norm of the scaled gradient before clipping; 0 when clipping is off
#define WUNET_HYPER_DECAY 4       // 1 - lr * weight_decay

// Sum of (gscale * g)^2 per block, in double.  Grid as for adam_kernel (blockIdx.y = tensor, blockIdx.x strides inside it); block
// (x, y) writes part[y * gridDim.x + x] - also when it had no element (0): the slots need no memset and adam_hyper_kernel adds
// every one of them.  Four trips' loads are in flight ahead of the first use (loss_partial_kernel); the terms are added in the
// one-trip loop's order.
static __global__ __launch_bounds__(WUNET_THREADS) void grad_sqnorm_partial_kernel(AdamTable T, float gscale, double* part)
{
    __shared__ double red[WUNET_WAVES];
    const int t = blockIdx.y;
    const float* g = T.g[t];
    const unsigned n = T.n[t];
    const double gs = (double)gscale;
    double s[1] = {0.0};
    const size_t stride = (size_t)gridDim.x * WUNET_THREADS;
    size_t i = (size_t)blockIdx.x * WUNET_THREADS + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {
        float e[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) e[u] = g[i + u * stride];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const double x = gs * (double)e[u]; s[0] += x * x; }
    }
    for (; i < n; i += stride) { const double x = gs * (double)g[i]; s[0] += x * x; }
    block_sum<1>(s, red);
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s[0];
}

// The step's scalars, one block: the bias-corrected step size lr / (1 - b1^t) and sqrt(1 - b2^t) in double like torch's host
// arithmetic.  step_dev != nullptr: the counter lives on the device (*step_dev += 1, so a captured graph replays the right bias
// corrections), otherwise `step` is the host's count.  lr_dev != nullptr: the learning rate is read from device memory (a double:
// lr / bc1 then has the bits of the host path).  n_part > 0: the n_part partial sums of grad_sqnorm_partial_kernel are added in a
// fixed order in double (thread k takes k, k + 256, ...; then block_sum's tree), norm = sqrt(sum) and
// clip = min(1, max_norm / (norm + 1e-6)) - clip_grad_norm_'s formula, in double, rounded to float once; a non-finite norm
// propagates as in torch (error_if_nonfinite=False): inf gives clip 0, NaN gives NaN.  The branch on n_part is uniform: without
// partial sums nothing meets at a barrier and a block of ONE thread does (the plain step's launch).  optional_slots false: the
// hyper buffer is wunet_adam_step's 2 floats and nothing is written behind them.
static __global__ __launch_bounds__(WUNET_THREADS) void adam_hyper_kernel(long long* step_dev, long long step, double lr, const double* lr_dev,
                                                                    double beta1, double beta2, double weight_decay, double max_norm,
                                                                    const double* part, int n_part, float* hyper, bool optional_slots)
{
    __shared__ double red[WUNET_WAVES];
    double s[1] = {0.0};
    if (n_part > 0) {
        int r = threadIdx.x;
        for (; r + 3 * WUNET_THREADS < n_part; r += 4 * WUNET_THREADS) {
            double e[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) e[u] = part[r + u * WUNET_THREADS];
#pragma unroll
            for (int u = 0; u < 4; ++u) s[0] += e[u];
        }
        for (; r < n_part; r += WUNET_THREADS) s[0] += part[r];
        block_sum<1>(s, red);
    }
    if (threadIdx.x != 0) return;
    long long t = step;
    if (step_dev) {
        t = *step_dev + 1;
        *step_dev = t;
    }
    if (lr_dev) lr = *lr_dev;
    const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
    hyper[WUNET_HYPER_STEP_SIZE] = (float)(lr / bc1);
    hyper[WUNET_HYPER_BC2_SQRT] = (float)sqrt(bc2);
    if (!optional_slots) return;
    double norm = 0.0, clip = 1.0;
    if (n_part > 0) {
        norm = sqrt(s[0]);
        const double c = max_norm / (norm + 1e-6);
        clip = c > 1.0 ? 1.0 : c;                   // (a NaN stays: torch.clamp(max=1) keeps it too)
    }
    hyper[WUNET_HYPER_CLIP] = (float)clip;
    hyper[WUNET_HYPER_NORM] = (float)norm;
    hyper[WUNET_HYPER_DECAY] = (float)(1.0 - lr * weight_decay);
}

// The last line of the update, p - step_size * q, as ONE fma on the device (the product is not rounded); the emulator build rounds
// it (its -ffp-contract=off stands for every line).
__device__ __forceinline__ float adam_update(float p, float step_size, float q)
{
#ifdef WUNET_EMU
    return p - step_size * q;
#else
    return __builtin_fmaf(-step_size, q, p);
#endif
}

// One launch of the update: blockIdx.y = tensor, blockIdx.x strides inside it.  torch's single-tensor order:
// m.lerp_(g, 1-b1); v = v*b2 + (1-b2)*g*g; denom = sqrt(v)/sqrt(1-b2^t) + eps; p -= (lr/(1-b1^t)) * m/denom.
// The roundings are asked for here and not left to the compiler: contraction is off in the loop, so every product of the two moment
// lines is rounded as torch's separate multiplies and adds round it, and torch.optim.AdamW's decayed parameter p * decay is rounded
// to float before the update is subtracted, never fused into it; the one fma is adam_update's.
// gscale: the gradient is multiplied by it first (1/world_size of the data-parallel average folded into the step: the same rounding
// as a separate g.mul_(1/world) pass); no multiply when the factor is exactly 1.  The gradient itself is NOT modified
// (clip_grad_norm_ scales it in place; the fused step does not pay that write).
// hyper == nullptr: step_size and bc2_sqrt are the arguments (computed on the host).  Otherwise they come from slots 0 and 1 of the
// hyper buffer (adam_hyper_kernel), and with optional_slots the clip factor (gi = g * (gscale * clip)) and the decay from theirs;
// without it nothing behind slot 1 is read.
static __global__ __launch_bounds__(WUNET_THREADS) void adam_kernel(AdamTable T, float one_minus_b1, float b2, float one_minus_b2,
                                                              float bc2_sqrt, float eps, float step_size, float gscale,
                                                              const float* hyper, bool optional_slots)
{
    float factor = gscale, decay = 1.0f;
    if (hyper) {
        step_size = hyper[WUNET_HYPER_STEP_SIZE]; bc2_sqrt = hyper[WUNET_HYPER_BC2_SQRT];
        if (optional_slots) { factor = gscale * hyper[WUNET_HYPER_CLIP]; decay = hyper[WUNET_HYPER_DECAY]; }
    }
    const int t = blockIdx.y;
    float* p = T.p[t];
    const float* g = T.g[t];
    float* m = T.m[t];
    float* v = T.v[t];
    const unsigned n = T.n[t];
    for (unsigned i = blockIdx.x * WUNET_THREADS + threadIdx.x; i < n; i += gridDim.x * WUNET_THREADS) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
        const float gi = factor == 1.0f ? g[i] : g[i] * factor;
        float mi = m[i], vi = v[i];
        mi = mi + one_minus_b1 * (gi - mi);
        vi = vi * b2 + one_minus_b2 * gi * gi;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        float pi = p[i];
        if (decay != 1.0f) pi = pi * decay;
        p[i] = adam_update(pi, step_size, mi / denom);
    }
}
