// dL/d(input waveform) (wunet_backward_input, include/wunet_hip.h).  model/unet_basic.py:77-100 reads the input in two places:
//   dx[b,t] = wh[C] gh[b,t]                                             (head: cat([o, input]) -> 1x1 conv; gh from head_bwd_kernel)
//           + sum_{c<C} sum_{k<15} W0[c,0,k] g_z0[b,c,t+7-k]            (encoder.0: Cin = 1, 15 taps, padding 7; g_z0 zero outside [0, Lt))
// g_z0 = k1 g + k2 z + k3 is encoder.0's gradient at its conv output.  The first layer's backward leaves it in one of three forms
// (wunet_backward.cpp: first_layer_gz_source), a compile-time mode here like gz_split_h3_kernel's GZ_* modes:
//   IG_ENC  nothing stored (pass_a_kernel<.., E0>): g is rebuilt from the consumers' data gradients - the skip rows of the last decoder
//           layer plus encoder.1's, zero-stuffed onto the even positions, times LeakyReLU' (WunetEncSrc, wunet_lrelu_bwd: what pass_a_kernel<A_ENC> calls) - then k1..k3
//   IG_G    g stored (the weight gradient forms g_z while it stages its chunks): k1..k3 applied here
//   IG_GZ   g_z stored (gz_materialize_kernel in place, or pass A's fused finalize)
// One block: WUNET_IG_TP positions of one row, four per thread.  WUNET_IG_CC channels at a time are formed into LDS with the 7-sample
// halo on either side (8: whole float4s); the 15-tap correlation runs on VALU from there (one output channel: nothing for MFMA).  Each
// output is one thread's sum in a fixed order - channels, taps, then the head term - so no atomics and the same bits on every run.
// HBM-bound: z, the stored or rebuilt gradient and gh read once (+ 16 / WUNET_IG_TP of halo), the caller's Tt samples written.
#pragma once
#include "wunet_dev.h"

enum { IG_ENC = 0, IG_G = 1, IG_GZ = 2 };
#define WUNET_IG_TP (4 * WUNET_THREADS)           // positions per block
#define WUNET_IG_CC 8                              // channels per LDS stage
#define WUNET_IG_ROW (WUNET_IG_TP + 16)            // one staged channel: positions t0 - 8 .. t0 + TP + 7

struct InputGradArgs {
    const float* z;                  // [B][C][L] encoder.0's raw conv output
    const float* k1; const float* k2; const float* k3;     // its BatchNorm-backward coefficients (frozen: k2 = k3 = 0)
    const float* g;                  // IG_G: g [B][C][L];  IG_GZ: g_z [B][C][L]
    const float* a; const float* s;  // IG_ENC: the layer's BatchNorm scale / shift (LeakyReLU' from a z + s)
    WunetEncSrc enc;                 // IG_ENC: the skip rows of the last decoder layer's data gradient, encoder.1's data gradient
    const float* w0;                 // encoder.0's conv weight [C][1][15]
    const float* wh;                 // head weight [1][C+1][1]: wh[C] multiplies the input
    const float* gh;                 // [B][L] head gradient before its 1x1 conv
    float* dx;                       // out [B][Tt]
    int B, C, L, Lt, Tt;
    int vec;                         // dx is 16-byte aligned and Tt a multiple of 4: float4 stores
};

template <int MODE>
__global__ __launch_bounds__(WUNET_THREADS) void input_grad_kernel(InputGradArgs A)
{
    __shared__ wunet_f4 tile4[WUNET_IG_CC * WUNET_IG_ROW / 4];
    float* const tile = reinterpret_cast<float*>(tile4);
    const int tid = threadIdx.x, b = blockIdx.y;
    const int t0 = blockIdx.x * WUNET_IG_TP;

    // g_z of channel c at positions p .. p + 3 (p a multiple of 4, L too: the four lie wholly inside [0, L) or wholly outside).  The loads
    // are unconditional (clamped index) and the value of a quad outside the row is dropped by a select, so a stage's loads issue together.
    auto form = [&](int c, int p) -> wunet_f4 {
        const bool ok = p >= 0 && p < A.L;
        const int pc = ok ? p : 0;
        const size_t i = ((size_t)b * A.C + c) * A.L + pc;
        wunet_f4 gz;
        if (MODE == IG_GZ) {
            gz = wunet_ld4(A.g + i);
        } else {
            const wunet_f4 z = wunet_ld4(A.z + i);
            wunet_f4 g;
            if (MODE == IG_G) g = wunet_ld4(A.g + i);
            else {
                const wunet_f4 d = wunet_enc_skip4(A.enc, b, c, A.L, pc);
                const float2 e = wunet_enc_half2(A.enc, b, A.C, c, A.L, pc);
                g = wunet_lrelu_bwd(A.a[c], A.s[c], z, wunet_enc_combine(d, e));
            }
            gz = wunet_gz(A.k1[c], A.k2[c], A.k3[c], g, z);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) gz[j] = (ok && p + j < A.Lt) ? gz[j] : 0.0f;      // (zero padding of the conv; no gradient in the row padding)
        return gz;
    };

    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int c0 = 0; c0 < A.C; c0 += WUNET_IG_CC) {
        const int nc = A.C - c0 < WUNET_IG_CC ? A.C - c0 : WUNET_IG_CC;
        // ---- stage: thread tid forms positions t0 + 4 tid .. + 3 of every channel of the stage; threads < 4 CC the two halo quads on each side
        {
            wunet_f4 v[WUNET_IG_CC];
#pragma unroll
            for (int q = 0; q < WUNET_IG_CC; ++q) v[q] = form(c0 + (q < nc ? q : 0), t0 + 4 * tid);
#pragma unroll
            for (int q = 0; q < WUNET_IG_CC; ++q)
                if (q < nc) wunet_st4(tile + q * WUNET_IG_ROW + 8 + 4 * tid, v[q]);
            if (tid < 4 * WUNET_IG_CC) {
                const int q = tid >> 2, h = tid & 3;
                const int at = h < 2 ? 4 * h : WUNET_IG_TP + 8 + 4 * (h - 2);             // staged index: 0, 4 | TP + 8, TP + 12
                if (q < nc) wunet_st4(tile + q * WUNET_IG_ROW + at, form(c0 + q, t0 - 8 + at));
            }
        }
        __syncthreads();
        // ---- correlate: output t0 + 4 tid + j reads staged indices 4 tid + j + 15 - k (k = 0 .. 14), i.e. 4 tid + 1 .. 4 tid + 18
        for (int q = 0; q < nc; ++q) {
            const float* row = tile + q * WUNET_IG_ROW + 4 * tid;
            float xs[20];
#pragma unroll
            for (int u = 0; u < 5; ++u) {
                const wunet_f4 t = wunet_ld4(row + 4 * u);
                xs[4 * u] = t[0]; xs[4 * u + 1] = t[1]; xs[4 * u + 2] = t[2]; xs[4 * u + 3] = t[3];
            }
            const float* w = A.w0 + (size_t)(c0 + q) * 15;
#pragma unroll
            for (int k = 0; k < 15; ++k) {
                const float wk = w[k];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = fmaf(wk, xs[j + 15 - k], acc[j]);
            }
        }
        __syncthreads();
    }
    // ---- the head term, then the caller's samples
    const int t = t0 + 4 * tid;
    if (t >= A.Tt) return;
    const float whin = A.wh[A.C];
    const wunet_f4 gh = wunet_ld4(A.gh + (size_t)b * A.L + t);          // (t < Tt <= L, both t and L multiples of 4)
    float* out = A.dx + (size_t)b * A.Tt + t;
    wunet_f4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = fmaf(whin, gh[j], acc[j]);
    if (A.vec) wunet_st4(out, o);
    else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (t + j < A.Tt) out[j] = o[j];
    }
}
