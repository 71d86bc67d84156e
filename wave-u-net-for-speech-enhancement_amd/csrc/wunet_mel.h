// Multi-scale log-mel spectrogram loss (include/wunet_hip.h: wunet_mel_*; HiFi-GAN's mel loss, the multi-scale mel loss of DAC /
// EnCodec-style codecs) of one resolution, forward and backward, on the two GEMMs of wunet_stft.h - same basis, same framing, same
// tiles - with a second, small GEMM against a filterbank Phi [n_mels][BP] between them.  Per bin and per mel cell of either signal:
//   P = re^2 + im^2,  Pc = max(P, clamp),  S = Pc^(power / 2),  m[f][j] = sum_b Phi[j][b] S[f][b],  l = ln max(m, floor)
//   term = log_weight |l_c - l_e| + lin_weight |m_c - m_e|
//   mel_spec_kernel      stft_fwd_kernel's grid and main loop (dft_tile_gemm, StftFrameLoader); the epilogue writes S of each signal as a
//                        plane [M][BP] (padding columns 0) and, for the backward, re_e and im_e; no sums
//   mel_proj_kernel      GEMM [M frames][bins] x Phi^T on v_mfma_f32_16x16x4_f32: one block owns 16 frames x ALL mel cells of both signals;
//                        the epilogue takes the logs in double and adds the two sums into the block's partial; saves m_c, m_e [M][MP]
//   cspec_final_kernel   (wunet_cspec.h) ONE block: the partials of every resolution in block order -> the loss, the gradient scales
//   mel_proj_bwd_kernel  the transposed projection dS[f][b] = sum_j g[f][j] Phi[j][b]; g is formed in the loader from m_c, m_e
//   mel_bwd_kernel       stft_bwd_kernel's adjoint GEMM (dft_adjoint_gemm) with the bin gradient of (re_e, im_e, dS)
//   (overlap-add)        stft_ola_kernel, unchanged
// A frame's mel cells sum over all bins of the frame, so the loss cannot be formed in the DFT epilogue: S goes once through memory.
// Both signals run through the same instructions: equal signals give equal m and exact zeros in loss and gradient.  fp32 operands and
// MFMA accumulation; the logs, every sum and every coefficient in double; no atomics: bit-identical run to run.
#pragma once
#include "wunet_cspec.h"

#define WUNET_MEL_MAX 128            // == WUNET_MEL_MAX_FILTERS: mel cells per frame, eight 16-column tiles per wave
#define WUNET_MEL_FM 16              // frames per block of the projection (every wave takes all of them)
#define WUNET_MEL_KT 32              // ... its K tile (eight MFMA steps)
#define WUNET_MEL_AS 34              // ... LDS row stride of its A tile: 34 i + q (i < 16, q < 4) meets a bank at most twice
#define WUNET_MEL_PLANES 3           // saved [3][M][BP]: re_e, im_e, dS (written by the backward), then [2][M][MP]: m_c, m_e

// The one definition of the saved buffer's layout for the kernels and the launcher (floats).
struct MelLayout {
    size_t plane, mplane;            // M * BP, M * MP
    __host__ __device__ MelLayout(unsigned M, int BP, int MP) : plane((size_t)M * BP), mplane((size_t)M * MP) {}
    __host__ __device__ size_t re() const { return 0; }
    __host__ __device__ size_t im() const { return plane; }
    __host__ __device__ size_t ds() const { return 2 * plane; }
    __host__ __device__ size_t mc() const { return WUNET_MEL_PLANES * plane; }
    __host__ __device__ size_t me() const { return WUNET_MEL_PLANES * plane + mplane; }
    __host__ __device__ size_t floats() const { return WUNET_MEL_PLANES * plane + 2 * mplane; }
};

// S = max(P, clamp)^(power / 2) from stft_power's bits: the forward of both signals and nothing else forms it
__device__ __forceinline__ float mel_spec(float re, float im, float clamp, int power)
{
    const float pc = fmaxf(stft_power(re, im), clamp);
    return power == 2 ? pc : sqrtf(pc);
}

struct MelSpecArgs {
    StftFwdArgs S;          // the frames and the GEMM, as stft_fwd_kernel reads them; part and mag_out unused; saved = nullptr or the
                            // saved buffer (MelLayout: re_e, im_e are written here)
    float* spec;            // [NSIG][M][BP]: S_e, then S_c
    int power;              // 1 or 2
};

// grid (M / 64 rounded up, BP / 32): one block owns 64 frames x 32 bins.  PAIR: both signals; else `e` alone.
template <bool PAIR>
static __global__ __launch_bounds__(WUNET_THREADS) void mel_spec_kernel(MelSpecArgs C)
{
    constexpr int NSIG = PAIR ? 2 : 1;
    __shared__ __attribute__((aligned(16))) float As[NSIG * WUNET_STFT_FM * WUNET_STFT_AS];
    __shared__ __attribute__((aligned(16))) float Bs[WUNET_STFT_KT * WUNET_STFT_BS];
    const StftFwdArgs& A = C.S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
    const unsigned m0 = blockIdx.x * WUNET_STFT_FM;
    const int b0 = blockIdx.y * WUNET_STFT_BN;
    wunet_f4 acc[NSIG][2][2];                    // [signal: e, c][re, im][column tile]
    dft_tile_gemm<NSIG>(StftFrameLoader<NSIG>(A, m0), A.basis, A.BP, b0, A.k0, A.k1, As, Bs, acc);
    // ---- epilogue: D[row = 4 lq + r][col = li] of the wave's 16 frames
    const MelLayout L(A.M, A.BP, 0);             // (re_e and im_e lie in front of everything that depends on MP)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int b = b0 + nt * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned m = m0 + (unsigned)(wave * 16 + lq * 4 + r);
            if (m >= A.M) continue;
            const size_t o = (size_t)m * A.BP + b;
            const bool live = b < A.bins;                                // (the padding columns: 0, whatever the clamp)
#pragma unroll
            for (int s = 0; s < NSIG; ++s) C.spec[s * L.plane + o] = live ? mel_spec(acc[s][0][nt][r], acc[s][1][nt][r], A.clamp, C.power) : 0.0f;
            if (A.saved) {                                               // (re = im = 0 in the padding columns)
                A.saved[L.re() + o] = acc[0][0][nt][r];
                A.saved[L.im() + o] = acc[0][1][nt][r];
            }
        }
    }
}

struct MelProjArgs {
    const float* spec;      // [NSIG][M][BP]: S_e, then S_c
    const float* filt;      // Phi [n_mels][BP], padding columns 0
    unsigned M;
    int BP, bins, n_mels, MP;   // MP = n_mels rounded up to 16
    double floor;
    double* part;           // [blocks][2]: sum |l_c - l_e|, sum |m_c - m_e|                       (PAIR)
    float* saved;           // nullptr or the saved buffer (MelLayout: m_c, m_e are written here)  (PAIR)
    float* mel_out;         // [M][n_mels]: m_e, or ln max(m_e, floor) where floor > 0             (single signal)
};

// grid M / 16 rounded up: one block owns WUNET_MEL_FM = 16 frames x all MP mel cells of both signals; every wave multiplies the same
// 16 frames, wave w by the column tiles w and w + 4 of Phi^T.  (64 frames per block - one frame tile per wave, all column tiles in
// every wave - left a few dozen blocks on the device at 64 x 16384, each with 64 MFMAs per wave and K tile in a row.)  K = the BP
// bins in tiles of WUNET_MEL_KT = 32: As[signal][16 frames][32 bins] (stride WUNET_MEL_AS), Bs[32 bins][MP] (Phi's tile transposed
// on its way into LDS, stride WUNET_STFT_BWS); the next tile's global loads are issued before the MFMAs of the current one.
// Loader roles.  A: tid < 128 NSIG: signal tid >> 7, frame (tid >> 3) & 15, four bins from (tid & 7) * 4.  B: piece = tid + 256 j:
// filter piece >> 3 (those below MP), four bins from (piece & 7) * 4.
template <bool PAIR>
static __global__ __launch_bounds__(WUNET_THREADS) void mel_proj_kernel(MelProjArgs A)
{
    constexpr int NSIG = PAIR ? 2 : 1;
    __shared__ __attribute__((aligned(16))) float As[NSIG * WUNET_MEL_FM * WUNET_MEL_AS];
    __shared__ __attribute__((aligned(16))) float Bs[WUNET_MEL_KT * WUNET_STFT_BWS];
    __shared__ double red[2 * WUNET_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
    const unsigned m0 = blockIdx.x * WUNET_MEL_FM;
    const size_t plane = (size_t)A.M * A.BP;
    const int nct = A.MP / 16;                                           // column tiles in use (block-uniform)
    const int as = tid >> 7, af = (tid >> 3) & 15, aq = (tid & 7) * 4;
    const unsigned am = m0 + (unsigned)af;
    const bool aload = as < NSIG, aok = aload && am < A.M;
    wunet_f4 ra = wunet_f4{0.f, 0.f, 0.f, 0.f}, rb[4];
    wunet_f4 acc[NSIG][2];                                               // [signal: e, c][column tile wave, wave + 4]
#pragma unroll
    for (int s = 0; s < NSIG; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[s][t] = wunet_f4{0.f, 0.f, 0.f, 0.f};
#define WUNET_MEL_LOAD(B0_)                                                                                          \
    do {                                                                                                             \
        if (aok) ra = wunet_ld4(A.spec + (size_t)as * plane + (size_t)am * A.BP + (B0_) + aq);                       \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                              \
            const int piece = tid + WUNET_THREADS * j, fj = piece >> 3;                                              \
            if (fj < A.MP) rb[j] = wunet_sel4(fj < A.n_mels, wunet_ld4(A.filt + (size_t)(fj < A.n_mels ? fj : 0) * A.BP + (B0_) + (piece & 7) * 4)); \
        }                                                                                                            \
    } while (0)
    WUNET_MEL_LOAD(0);
    for (int b0 = 0; b0 < A.BP; b0 += WUNET_MEL_KT) {
        __syncthreads();                                                 // the previous tile's reads are done
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (aload) As[(as * WUNET_MEL_FM + af) * WUNET_MEL_AS + aq + e] = ra[e];      // (rows beyond M: zeros)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int piece = tid + WUNET_THREADS * j;
                if ((piece >> 3) < A.MP) Bs[((piece & 7) * 4 + e) * WUNET_STFT_BWS + (piece >> 3)] = rb[j][e];
            }
        }
        __syncthreads();
        if (b0 + WUNET_MEL_KT < A.BP) WUNET_MEL_LOAD(b0 + WUNET_MEL_KT);
#pragma unroll
        for (int s4 = 0; s4 < WUNET_MEL_KT / 4; ++s4) {
            const int kk = s4 * 4 + lq;
            float a[NSIG];
#pragma unroll
            for (int s = 0; s < NSIG; ++s) a[s] = As[(s * WUNET_MEL_FM + li) * WUNET_MEL_AS + kk];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (wave + 4 * t < nct) {                                // (wave-uniform)
                    const float b = Bs[kk * WUNET_STFT_BWS + (wave + 4 * t) * 16 + li];
#pragma unroll
                    for (int s = 0; s < NSIG; ++s) acc[s][t] = wunet_mfma16(a[s], b, acc[s][t]);
                }
            }
        }
    }
#undef WUNET_MEL_LOAD
    // ---- epilogue: D[row = 4 lq + r][col = li] of the block's 16 frames x the wave's column tiles: whole cells
    double sum[2] = {0.0, 0.0};
    const MelLayout L(A.M, A.BP, A.MP);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        if (wave + 4 * t >= nct) continue;
        const int j = (wave + 4 * t) * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned m = m0 + (unsigned)(lq * 4 + r);
            if (m >= A.M) continue;
            const float me = acc[0][t][r];
            if (PAIR) {
                const float mc = acc[PAIR ? 1 : 0][t][r];
                if (j < A.n_mels) {
                    sum[0] += fabs(log(fmax((double)mc, A.floor) / fmax((double)me, A.floor)));     // l_c - l_e: one log
                    sum[1] += fabs((double)mc - (double)me);
                }
                if (A.saved) {                                           // (the padding columns too: Phi has no row there, m = 0)
                    A.saved[L.mc() + (size_t)m * A.MP + j] = mc;
                    A.saved[L.me() + (size_t)m * A.MP + j] = me;
                }
            } else if (j < A.n_mels) {
                A.mel_out[(size_t)m * A.n_mels + j] = A.floor > 0.0 ? (float)log(fmax((double)me, A.floor)) : me;
            }
        }
    }
    if (PAIR) {
        block_sum<2>(sum, red);
        if (tid == 0) {
            double* o = A.part + (size_t)blockIdx.x * 2;
            o[0] = sum[0]; o[1] = sum[1];
        }
    }
}

struct MelProjBwdArgs {
    float* saved;           // the saved buffer (MelLayout): m_c, m_e are read, dS is written
    const double* coefs;    // c_log, c_lin of this resolution
    const float* filt;      // Phi [n_mels][BP]
    unsigned M;
    int BP, n_mels, MP;
    double floor;
};

// d loss / d m_e of one cell: c_log sign(l_e - l_c) / m_e where m_e >= floor (torch.clamp passes a gradient there; l is monotone in
// max(m, floor), whose order gives the sign) + c_lin sign(m_e - m_c); sign(0) = 0
__device__ __forceinline__ float mel_cell_grad(float mc, float me, double floor, double c_log, double c_lin)
{
    const double dc = fmax((double)mc, floor), de = fmax((double)me, floor);
    double g = c_lin * (me > mc ? 1.0 : (me < mc ? -1.0 : 0.0));
    if ((double)me >= floor) g += c_log * (de > dc ? 1.0 : (de < dc ? -1.0 : 0.0)) / (double)me;
    return (float)g;
}

// grid (M / 64 rounded up, BP / 128 rounded up): one block owns 64 frames x 128 bins of dS = g x Phi (wave w: frames 16 w .. 16 w + 15,
// eight 16-column tiles - dft_adjoint_gemm's shape).  K = the mel cells in tiles of 16: Gs[64 frames][16 cells] (stride WUNET_STFT_AS),
// g formed from m_c, m_e on the way into LDS; Bs[16 cells][128 bins] (stride WUNET_STFT_BWS), Phi's rows as they lie in memory.
// Loader roles.  G: frame tid >> 2, four cells from (tid & 3) * 4.  B: piece = tid + 256 j: cell piece >> 5, four bins from (piece & 31) * 4.
static __global__ __launch_bounds__(WUNET_THREADS) void mel_proj_bwd_kernel(MelProjBwdArgs A)
{
    __shared__ __attribute__((aligned(16))) float Gs[WUNET_STFT_FM * WUNET_STFT_AS];
    __shared__ __attribute__((aligned(16))) float Bs[WUNET_STFT_KT * WUNET_STFT_BWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
    const unsigned m0 = blockIdx.x * WUNET_STFT_FM;
    const int bin0 = blockIdx.y * WUNET_STFT_BWN;
    const MelLayout L(A.M, A.BP, A.MP);
    const double c_log = A.coefs[0], c_lin = A.coefs[1];
    const unsigned am = m0 + (unsigned)(tid >> 2);
    const int aq = (tid & 3) * 4;
    const bool aok = am < A.M;
    wunet_f4 rc, re, rb[2];
    wunet_f4 acc[8];
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) acc[nt] = wunet_f4{0.f, 0.f, 0.f, 0.f};
#define WUNET_MEL_BLOAD(J0_)                                                                                         \
    do {                                                                                                             \
        const size_t o = (size_t)(aok ? am : 0u) * A.MP + (J0_) + aq;                                                \
        rc = wunet_sel4(aok, wunet_ld4(A.saved + L.mc() + o));                                                       \
        re = wunet_sel4(aok, wunet_ld4(A.saved + L.me() + o));                                                       \
        _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                              \
            const int piece = tid + WUNET_THREADS * j, fj = (J0_) + (piece >> 5), b = bin0 + (piece & 31) * 4;       \
            const bool ok = fj < A.n_mels && b < A.BP;                                                               \
            rb[j] = wunet_sel4(ok, wunet_ld4(A.filt + (size_t)(ok ? fj : 0) * A.BP + (ok ? b : 0)));                 \
        }                                                                                                            \
    } while (0)
    WUNET_MEL_BLOAD(0);
    for (int j0 = 0; j0 < A.MP; j0 += WUNET_STFT_KT) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) Gs[(tid >> 2) * WUNET_STFT_AS + aq + e] = mel_cell_grad(rc[e], re[e], A.floor, c_log, c_lin);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int piece = tid + WUNET_THREADS * j;
            wunet_st4(&Bs[(piece >> 5) * WUNET_STFT_BWS + (piece & 31) * 4], rb[j]);
        }
        __syncthreads();
        if (j0 + WUNET_STFT_KT < A.MP) WUNET_MEL_BLOAD(j0 + WUNET_STFT_KT);
#pragma unroll
        for (int s4 = 0; s4 < WUNET_STFT_KT / 4; ++s4) {
            const int kk = s4 * 4 + lq;
            const float a = Gs[(wave * 16 + li) * WUNET_STFT_AS + kk];
#pragma unroll
            for (int nt = 0; nt < 8; ++nt) acc[nt] = wunet_mfma16(a, Bs[kk * WUNET_STFT_BWS + nt * 16 + li], acc[nt]);
        }
    }
#undef WUNET_MEL_BLOAD
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) {
        const int b = bin0 + nt * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned m = m0 + (unsigned)(wave * 16 + lq * 4 + r);
            if (m < A.M && b < A.BP) A.saved[L.ds() + (size_t)m * A.BP + b] = acc[nt][r];
        }
    }
}

struct MelBwdArgs {
    const float* saved;     // the saved buffer: its first WUNET_MEL_PLANES planes [M][BP] are re_e, im_e, dS
    const double* coefs;    // (unused here: dS carries the scales)
    const float* basis;     // [N][2 BP]
    unsigned M, ktiles;     // ktiles: blocks along the window positions
    int N, BP, bins, k0, k1;
    float clamp;
    int power;
    float* scratch;         // [M][N], written for k0 <= k < k1
};

// The loader's view of the three planes (StftBinGrad's contract): (dRe, dIm) = dS power Pc^(power / 2 - 1) (re, im) where P >= clamp,
// nothing below it; P from stft_power, the forward's bits.  Rows beyond M load zeros: P = 0 lies below every clamp.
struct MelBinGrad {
    static constexpr int PLANES = WUNET_MEL_PLANES;
    float clamp;
    int power;
    __device__ __forceinline__ static float pad(int) { return 0.0f; }
    __device__ __forceinline__ void grad(const float (&r)[PLANES], float& dre, float& dim) const
    {
        const float p = stft_power(r[0], r[1]);
        dre = 0.0f; dim = 0.0f;
        if (p >= clamp) {
            const double f = power == 2 ? 2.0 * (double)r[2] : (double)r[2] / (double)sqrtf(p);
            dre = (float)(f * (double)r[0]);
            dim = (float)(f * (double)r[1]);
        }
    }
};

// grid ktiles * (M / 64 rounded up): stft_bwd_kernel's adjoint GEMM (dft_adjoint_gemm) with this loss's bins.
static __global__ __launch_bounds__(WUNET_THREADS) void mel_bwd_kernel(MelBwdArgs A)
{
    __shared__ __attribute__((aligned(16))) float Gs[WUNET_STFT_FM * WUNET_STFT_AS];
    __shared__ __attribute__((aligned(16))) float Bt[WUNET_STFT_KT * WUNET_STFT_BWS];
    dft_adjoint_gemm(MelBinGrad{A.clamp, A.power}, A.saved, A.basis, A.M, A.ktiles, A.N, A.BP, A.bins, A.k0, A.k1, A.scratch, Gs, Bt);
}
