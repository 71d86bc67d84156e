// Reductions over the 256-thread block, in one fixed order (bit-identical run to run): the closing step of the network's statistics
// kernels and of every loss, metric, mixer and optimiser kernel that sums or takes a maximum.
#pragma once
#include "wunet_dev.h"

// ---------------------------------------------------------------------------- block reduce helper
// sums N doubles over the 256-thread block; result valid in every thread.  red = N * WUNET_WAVES doubles of LDS.
// Butterfly inside each wave (no barrier), the four wave sums through LDS: two barriers instead of the nine of a 256-wide LDS tree -
// these reductions end kernels that are a few microseconds of pure latency (BatchNorm finalizes, split-K sums).  Fixed order.
template <int N>
__device__ __forceinline__ void block_sum(double (&a)[N], double* red)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) a[k] += wunet_shfl_xor_d(a[k], m);
    }
    __syncthreads();                           // (the previous user of red is done with it)
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) red[k * WUNET_WAVES + (tid >> 6)] = a[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k)
        a[k] = (red[k * WUNET_WAVES] + red[k * WUNET_WAVES + 1]) + (red[k * WUNET_WAVES + 2] + red[k * WUNET_WAVES + 3]);
}

// the two sums of the network's own kernels (BatchNorm finalizes, split-K sums, the head's backward)
__device__ __forceinline__ void block_sum2(double& a, double& b, double* red)
{
    double v[2] = {a, b};
    block_sum<2>(v, red);
    a = v[0]; b = v[1];
}

// max of two non-negative floats over the block (same LDS buffer, after a block_sum2); result valid in thread 0
__device__ __forceinline__ void block_max2(float& a, float& b, double* red)
{
    float* fr = reinterpret_cast<float*>(red);
    const int tid = threadIdx.x;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        a = fmaxf(a, wunet_shfl_xor(a, m));
        b = fmaxf(b, wunet_shfl_xor(b, m));
    }
    __syncthreads();
    if ((tid & 63) == 0) {
        fr[tid >> 6] = a;
        fr[WUNET_WAVES + (tid >> 6)] = b;
    }
    __syncthreads();
    a = fmaxf(fmaxf(fr[0], fr[1]), fmaxf(fr[2], fr[3]));
    b = fmaxf(fmaxf(fr[WUNET_WAVES], fr[WUNET_WAVES + 1]), fmaxf(fr[WUNET_WAVES + 2], fr[WUNET_WAVES + 3]));
}

// The closing reduction of pass A (pass_a_kernel, wunet_elementwise.h): two sums (three in HEAD mode) and two maxima over the block behind ONE
// barrier - butterflies inside each wave, the four waves' values through LDS, added in block_sum2's order (the same bits).  Rounds 1 - 6 ran
// block_sum2, block_max2 (and a second block_sum2 in HEAD mode) one after the other: four to seven barriers at the end of blocks that are only
// 4 - 8 loop trips long.  Sums valid in every thread, maxima too.  red: 5 * WUNET_WAVES doubles.
__device__ __forceinline__ void block_reduce_pass_a(double& s1, double& s2, double& s3, bool want3, float& mg, float& mz, double* red)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        s1 += wunet_shfl_xor_d(s1, m);
        s2 += wunet_shfl_xor_d(s2, m);
        if (want3) s3 += wunet_shfl_xor_d(s3, m);
        mg = fmaxf(mg, wunet_shfl_xor(mg, m));
        mz = fmaxf(mz, wunet_shfl_xor(mz, m));
    }
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
        red[w] = s1; red[WUNET_WAVES + w] = s2; red[2 * WUNET_WAVES + w] = s3;
        red[3 * WUNET_WAVES + w] = (double)mg; red[4 * WUNET_WAVES + w] = (double)mz;        // (a float survives the round trip through a double)
    }
    __syncthreads();
    s1 = (red[0] + red[1]) + (red[2] + red[3]);
    s2 = (red[WUNET_WAVES] + red[WUNET_WAVES + 1]) + (red[WUNET_WAVES + 2] + red[WUNET_WAVES + 3]);
    s3 = (red[2 * WUNET_WAVES] + red[2 * WUNET_WAVES + 1]) + (red[2 * WUNET_WAVES + 2] + red[2 * WUNET_WAVES + 3]);
    mg = fmaxf(fmaxf((float)red[3 * WUNET_WAVES], (float)red[3 * WUNET_WAVES + 1]), fmaxf((float)red[3 * WUNET_WAVES + 2], (float)red[3 * WUNET_WAVES + 3]));
    mz = fmaxf(fmaxf((float)red[4 * WUNET_WAVES], (float)red[4 * WUNET_WAVES + 1]), fmaxf((float)red[4 * WUNET_WAVES + 2], (float)red[4 * WUNET_WAVES + 3]));
}
