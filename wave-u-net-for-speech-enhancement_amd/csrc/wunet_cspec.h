// Power-law compressed spectral loss with a complex (phase-aware) term (include/wunet_hip.h: wunet_cspec_*; Braun & Tashev 2021) of one
// resolution, forward and backward, on the two GEMMs of wunet_stft.h - same basis, same framing, same tiles.  Per bin of either signal:
//   P = re^2 + im^2,  Pc = max(P, clamp),  s = Pc^((compress - 1) / 2),  A = s sqrt(Pc) = Pc^(compress / 2),  Z = (re, im) s
//   term = (1 - lambda) (A_c - A_e)^2 + lambda |Z_c - Z_e|^2
//   cspec_fwd_kernel    stft_fwd_kernel<true>'s grid and main loop (dft_tile_gemm<2>, StftFrameLoader<2>); the epilogue compresses both
//                       signals and adds the two sums of squares in double into the block's partial
//   cspec_final_kernel  ONE block: the partials of every resolution in block order -> the two means, the loss, the gradient scales
//   cspec_bwd_kernel    stft_bwd_kernel's adjoint GEMM (dft_adjoint_gemm); (dRe, dIm) of a bin from the five saved planes re_e, im_e, A_c, Re Z_c, Im Z_c
//   (overlap-add)       stft_ola_kernel, unchanged
// A and Z are rounded to float32 ONCE, by cspec_compress, and both kernels take their differences from those floats: the backward
// recomputes the enhanced side with the same function and meets the forward's bits, so equal signals give exact zeros in both.
// The powers (exp(h ln Pc) in double: h = 0 gives exactly 1), every sum and every coefficient in double; no atomics: bit-identical
// run to run.
#pragma once
#include "wunet_stft.h"

#define WUNET_CSPEC_NCOEF 4          // == WUNET_CSPEC_COEFS: the two gradient scales, the two term values per resolution
#define WUNET_CSPEC_PLANES 5         // saved [5][M][BP]: re_e, im_e, A_c, Re Z_c, Im Z_c

struct CspecPoint { float a, zr, zi; };

// One bin: p = re^2 + im^2 (stft_power's bits), s = max(p, clamp)^hs in double (hs = (compress - 1) / 2), root = sqrt(max(p, clamp));
// A = s root and Z = (re, im) s, each ONE double product rounded to float - nothing here that a compiler could contract differently
// in the two kernels that call it.
__device__ __forceinline__ CspecPoint cspec_compress(float re, float im, float clamp, double hs, float& p, double& s, double& root)
{
    p = stft_power(re, im);
    const double pc = (double)fmaxf(p, clamp);
    s = exp(hs * log(pc));
    root = sqrt(pc);
    CspecPoint q;
    q.a = (float)(s * root);
    q.zr = (float)((double)re * s);
    q.zi = (float)((double)im * s);
    return q;
}

struct CspecFwdArgs {
    StftFwdArgs S;          // the frames and the GEMM of the pair, as stft_fwd_kernel<true> reads them; here part = [blocks][2]:
                            // sum (A_c - A_e)^2, sum |Z_c - Z_e|^2; saved = nullptr or [WUNET_CSPEC_PLANES][M][BP]; mag_out unused
    double hs;              // (compress - 1) / 2
};

// grid (M / 64 rounded up, BP / 32): one block owns 64 frames x 32 bins of both signals.
static __global__ __launch_bounds__(WUNET_THREADS) void cspec_fwd_kernel(CspecFwdArgs C)
{
    __shared__ __attribute__((aligned(16))) float As[2 * WUNET_STFT_FM * WUNET_STFT_AS];
    __shared__ __attribute__((aligned(16))) float Bs[WUNET_STFT_KT * WUNET_STFT_BS];
    __shared__ double red[2 * WUNET_WAVES];
    const StftFwdArgs& A = C.S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
    const unsigned m0 = blockIdx.x * WUNET_STFT_FM;
    const int b0 = blockIdx.y * WUNET_STFT_BN;
    wunet_f4 acc[2][2][2];                       // [signal: e, c][re, im][column tile]
    dft_tile_gemm<2>(StftFrameLoader<2>(A, m0), A.basis, A.BP, b0, A.k0, A.k1, As, Bs, acc);
    // ---- epilogue: D[row = 4 lq + r][col = li] of the wave's 16 frames
    double sum[2] = {0.0, 0.0};
    const size_t plane = (size_t)A.M * A.BP;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int b = b0 + nt * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned m = m0 + (unsigned)(wave * 16 + lq * 4 + r);
            if (m >= A.M) continue;
            const float re = acc[0][0][nt][r], im = acc[0][1][nt][r];
            float p;
            double s, root;
            const CspecPoint e = cspec_compress(re, im, A.clamp, C.hs, p, s, root);
            const CspecPoint c = cspec_compress(acc[1][0][nt][r], acc[1][1][nt][r], A.clamp, C.hs, p, s, root);
            if (b < A.bins) {
                const double da = (double)c.a - (double)e.a, dr = (double)c.zr - (double)e.zr, di = (double)c.zi - (double)e.zi;
                sum[0] += da * da;
                sum[1] += dr * dr + di * di;
            }
            if (A.saved) {                                               // (the padding columns too: re = im = 0 there in both signals)
                const size_t o = (size_t)m * A.BP + b;
                A.saved[o] = re;
                A.saved[plane + o] = im;
                A.saved[2 * plane + o] = c.a;
                A.saved[3 * plane + o] = c.zr;
                A.saved[4 * plane + o] = c.zi;
            }
        }
    }
    block_sum<2>(sum, red);
    if (tid == 0) {
        double* o = A.part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        o[0] = sum[0]; o[1] = sum[1];
    }
}

struct CspecFinalArgs {
    const double* part[WUNET_STFT_MAX_RES];
    unsigned nparts[WUNET_STFT_MAX_RES];
    double count[WUNET_STFT_MAX_RES];      // rows * F * bins (wunet_mel.h: rows * F * n_mels)
    int n_res;
    double w0, w1;                         // the weights of the two sums: 1 - complex_weight, complex_weight (wunet_mel.h: log_weight, lin_weight)
    float* loss;
    double* coefs;                         // nullptr or [n_res][WUNET_CSPEC_NCOEF]
};

// ONE block over the table of resolutions, stft_final_kernel's order of sums.  mag = mean (A_c - A_e)^2, cplx = mean |Z_c - Z_e|^2;
// coefs = w0 / (n_res count), w1 / (n_res count), mag, cplx.  The loss is accumulated over the resolutions in double and rounded
// once.  Also the finalize of the mel loss (wunet_mel.h), whose two sums are |l_c - l_e| and |m_c - m_e|.
static __global__ __launch_bounds__(WUNET_THREADS) void cspec_final_kernel(CspecFinalArgs A)
{
    __shared__ double red[2 * WUNET_WAVES];
    const int tid = threadIdx.x;
    double total = 0.0;
    for (int i = 0; i < A.n_res; ++i) {
        double sum[2] = {0.0, 0.0};
        for (unsigned p = tid; p < A.nparts[i]; p += WUNET_THREADS) {
            const double* q = A.part[i] + (size_t)p * 2;
            sum[0] += q[0]; sum[1] += q[1];
        }
        block_sum<2>(sum, red);
        const double mag = sum[0] / A.count[i], cplx = sum[1] / A.count[i];
        total += A.w0 * mag + A.w1 * cplx;
        if (tid == 0 && A.coefs) {
            double* o = A.coefs + (size_t)i * WUNET_CSPEC_NCOEF;
            o[0] = A.w0 / ((double)A.n_res * A.count[i]);
            o[1] = A.w1 / ((double)A.n_res * A.count[i]);
            o[2] = mag;
            o[3] = cplx;
        }
    }
    if (tid == 0) *A.loss = (float)(total / (double)A.n_res);
}

struct CspecBwdArgs {
    const float* saved;     // [WUNET_CSPEC_PLANES][M][BP]
    const double* coefs;    // the two gradient scales of this resolution
    const float* basis;     // [N][2 BP]
    unsigned M, ktiles;     // ktiles: blocks along the window positions
    int N, BP, bins, k0, k1;
    float clamp;
    double compress, hs;    // hs = (compress - 1) / 2
    float* scratch;         // [M][N], written for k0 <= k < k1
};

// d loss / d (re, im) of one bin.  With dA = A_c - A_e, dZ = Z_c - Z_e, k1 / k2 the two scales:
//   d/d re = -2 [ k1 dA dA_e/d re + k2 (Re dZ (s + re ds/d re) + Im dZ im ds/d re) ],
//   dA_e/d re = compress (s / sqrt(P)) re,  ds/d re = (compress - 1) (s / P) re  where P >= clamp, both 0 below it (torch.clamp: s and
//   A_e are constants there and Z_e is linear in (re, im)).
__device__ __forceinline__ void cspec_bin_grad(float re, float im, float ac, float zrc, float zic, float clamp, double compress, double hs,
                                               double k1, double k2, float& dre, float& dim)
{
    float p;
    double s, root;
    const CspecPoint e = cspec_compress(re, im, clamp, hs, p, s, root);
    const double dzr = (double)zrc - (double)e.zr, dzi = (double)zic - (double)e.zi;
    double u = 0.0;
    if (p >= clamp) {
        const double da = (double)ac - (double)e.a, inv = 1.0 / root;
        u = (k1 * compress * da + k2 * (compress - 1.0) * inv * (dzr * (double)re + dzi * (double)im)) * (s * inv);
    }
    dre = (float)(-2.0 * (u * (double)re + k2 * s * dzr));
    dim = (float)(-2.0 * (u * (double)im + k2 * s * dzi));
}

// The loader's view of the five planes (StftBinGrad's contract): rows beyond M load zeros in every plane - a zero gradient.
struct CspecBinGrad {
    static constexpr int PLANES = WUNET_CSPEC_PLANES;
    float clamp;
    double compress, hs, k1, k2;
    __device__ __forceinline__ static float pad(int) { return 0.0f; }
    __device__ __forceinline__ void grad(const float (&r)[PLANES], float& dre, float& dim) const
    {
        cspec_bin_grad(r[0], r[1], r[2], r[3], r[4], clamp, compress, hs, k1, k2, dre, dim);
    }
};

// grid ktiles * (M / 64 rounded up): stft_bwd_kernel's adjoint GEMM (dft_adjoint_gemm) with this loss's bins.
static __global__ __launch_bounds__(WUNET_THREADS) void cspec_bwd_kernel(CspecBwdArgs A)
{
    __shared__ __attribute__((aligned(16))) float Gs[WUNET_STFT_FM * WUNET_STFT_AS];
    __shared__ __attribute__((aligned(16))) float Bt[WUNET_STFT_KT * WUNET_STFT_BWS];
    dft_adjoint_gemm(CspecBinGrad{A.clamp, A.compress, A.hs, A.coefs[0], A.coefs[1]}, A.saved, A.basis, A.M, A.ktiles, A.N, A.BP, A.bins, A.k0, A.k1,
                     A.scratch, Gs, Bt);
}
