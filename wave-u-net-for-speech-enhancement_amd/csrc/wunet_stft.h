// Multi-resolution STFT loss (include/wunet_hip.h: wunet_stft_*): spectral convergence + log-magnitude L1 of one resolution
// (n_fft = N, hop = H, window W <= N), forward and backward, as two GEMMs against a windowed DFT basis.
//   stft_basis_kernel   basis[N][2 BP]: row k = w[k] cos(2 pi k b / N) for b < BP, then -w[k] sin(..) for b < BP (planar; BP = the bins
//                       N/2 + 1 rounded up to 32, the padding columns and the rows outside the window are 0)
//   stft_fwd_kernel     implicit GEMM [rows F][N] x basis on v_mfma_f32_16x16x4_f32: A = the frames, read from the waveform with the
//                       reflect padding and the frame overlap resolved in the loader; one block owns 64 frames x 32 bins of BOTH signals;
//                       the epilogue forms the magnitudes and one partial (three doubles) of the block's sums
//   stft_final_kernel   ONE block: the partials of every resolution in block order -> sc, mag, the loss, the gradient coefficients
//   stft_bwd_kernel     adjoint GEMM [rows F][2 bins] x basis^T -> scratch [rows F][N]; A is formed in the loader from the saved spectra
//                       (dft_adjoint_gemm: the loop is shared with wunet_cspec.h, which brings its own bins)
//   stft_ola_kernel     overlap-add as a gather: every sample sums its frames' contributions in frame order, the reflected ones too
// fp32 operands and accumulation, every reduction and coefficient in double, no atomics: bit-identical run to run.
#pragma once
#include "wunet_reduce.h"

#define WUNET_STFT_FM 64             // frames per block (one 16-row MFMA tile per wave)
#define WUNET_STFT_BN 32             // forward: bins per block (two 16-column tiles, cos and -sin each)
#define WUNET_STFT_KT 16             // K tile of both GEMMs (four MFMA steps)
#define WUNET_STFT_AS 18             // LDS row stride of an A tile: 18 i + q (i < 16, q < 2) hits 32 different banks
#define WUNET_STFT_BS 80             // ... of the forward's B tile [16][64]: 80 q + j (q < 2, j < 16) likewise (80 = 16 mod 32)
#define WUNET_STFT_BWN 128           // backward: output samples (window positions k) per block, eight 16-column tiles per wave
#define WUNET_STFT_BWS 144           // ... row stride of its B tile [16][128] (144 = 16 mod 32)
#define WUNET_STFT_MAX_RES 8         // == WUNET_STFT_MAX_RESOLUTIONS
#define WUNET_STFT_NCOEF 4           // == WUNET_STFT_COEFS: a, b, sc, mag per resolution

#ifdef WUNET_EMU
__device__ __forceinline__ void wunet_sincospi_d(double x, double* s, double* c)
{
    const double pi = 3.14159265358979323846;
    *s = sin(pi * x);
    *c = cos(pi * x);
}
#else
__device__ __forceinline__ void wunet_sincospi_d(double x, double* s, double* c) { sincospi(x, s, c); }
#endif

// re^2 + im^2 with ONE stated contraction: the forward and the backward must get the same bits whatever the compiler fuses elsewhere
__device__ __forceinline__ float stft_power(float re, float im) { return fmaf(re, re, im * im); }

// grid (2 BP / 256 rounded up, N): one basis row per blockIdx.y.  left = (N - W) / 2: the window's first sample (torch.stft's centring).
static __global__ __launch_bounds__(WUNET_THREADS) void stft_basis_kernel(int N, int W, int BP, float* basis)
{
    const int k = blockIdx.y, col = blockIdx.x * WUNET_THREADS + threadIdx.x;
    if (col >= 2 * BP) return;
    const int b = col < BP ? col : col - BP, j = k - (N - W) / 2;
    float v = 0.0f;
    if (b <= N / 2 && j >= 0 && j < W) {
        double s, c;
        wunet_sincospi_d(2.0 * (double)j / (double)W, &s, &c);
        const double w = 0.5 - 0.5 * c;                               // periodic Hann
        const int ph = (int)(((long long)k * b) % N);                 // the phase from (k b) mod N in integers: exact for any k b
        wunet_sincospi_d(2.0 * (double)ph / (double)N, &s, &c);
        v = (float)(col < BP ? w * c : -(w * s));
    }
    basis[(size_t)k * 2 * BP + col] = v;
}

struct StftFwdArgs {
    const float* c;         // clean [rows][T]        (unused by the single-signal instantiation)
    const float* e;         // enhanced [rows][T]
    const float* basis;     // [N][2 BP]
    size_t T;
    unsigned M, F;          // M = rows * F frames in all
    int N, H, BP, bins;
    int k0, k1;             // the window's support rounded out to WUNET_STFT_KT
    float clamp;
    double* part;           // [blocks][3]: sum (S_c - S_e)^2, sum S_c^2, sum |ln S_c - ln S_e|
    float* saved;           // nullptr or [3][M][BP]: re_e, im_e, S_c
    float* mag_out;         // nullptr or [M][bins]: S_e
};

// The main loop of one block's DFT GEMM: acc[signal][re, im][column tile] = sum over k_begin <= k < k_end (multiples of WUNET_STFT_KT) of
// A[signal][64 frames][k] x basis[k][bins b0 .. b0 + 31, cos | -sin]; basis rows are 2 BP floats.  A tile As[signal][64 frames][16 k],
// B tile Bs[16 k][32 cos | 32 -sin]; the next tile's global loads are issued before the MFMAs of the current one and stored to LDS
// behind them.  Loader roles.  A: k = tid & 15, frames (tid >> 4) + 16 j - loader.load(kt, ra) fetches ra[signal][j] at k = kt + (tid & 15).
// B: row tid >> 4, four columns from (tid & 15) * 4.  Every thread of the block takes part (two barriers per K tile).
template <int NSIG, class Loader>
__device__ __forceinline__ void dft_tile_gemm(const Loader& loader, const float* basis, int BP, int b0, int k_begin, int k_end, float* As, float* Bs,
                                              wunet_f4 (&acc)[NSIG][2][2])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
    const int ak = tid & 15, bk = tid >> 4, bc = (tid & 15) * 4;
    const float* bsrc = basis + (size_t)bk * 2 * BP + (bc < WUNET_STFT_BN ? b0 + bc : BP + b0 + bc - WUNET_STFT_BN);
    float ra[NSIG][4];
    wunet_f4 rb;
#pragma unroll
    for (int s = 0; s < NSIG; ++s)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) acc[s][p][nt] = wunet_f4{0.f, 0.f, 0.f, 0.f};
    loader.load(k_begin, ra);
    rb = wunet_ld4(bsrc + (size_t)k_begin * 2 * BP);
    for (int kt = k_begin; kt < k_end; kt += WUNET_STFT_KT) {
        __syncthreads();                                               // the previous tile's reads are done
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ml = (tid >> 4) + 16 * j;
#pragma unroll
            for (int s = 0; s < NSIG; ++s) As[(s * WUNET_STFT_FM + ml) * WUNET_STFT_AS + ak] = ra[s][j];
        }
        wunet_st4(&Bs[bk * WUNET_STFT_BS + bc], rb);
        __syncthreads();
        if (kt + WUNET_STFT_KT < k_end) {
            loader.load(kt + WUNET_STFT_KT, ra);
            rb = wunet_ld4(bsrc + (size_t)(kt + WUNET_STFT_KT) * 2 * BP);
        }
#pragma unroll
        for (int s4 = 0; s4 < WUNET_STFT_KT / 4; ++s4) {
            const int kk = s4 * 4 + lq;
            float a[NSIG];
#pragma unroll
            for (int s = 0; s < NSIG; ++s) a[s] = As[(s * WUNET_STFT_FM + wave * 16 + li) * WUNET_STFT_AS + kk];
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const float b = Bs[kk * WUNET_STFT_BS + p * WUNET_STFT_BN + nt * 16 + li];
#pragma unroll
                    for (int s = 0; s < NSIG; ++s) acc[s][p][nt] = wunet_mfma16(a[s], b, acc[s][p][nt]);
                }
        }
    }
}

// A of the STFT: frame f of a row starts at f H - N / 2 of the waveform, reflect-padded.  Signal 0 = enhanced, 1 = clean.
template <int NSIG>
struct StftFrameLoader {
    const float* x[2];
    size_t abase[4];
    long long apos[4], Tl;
    bool aok[4];
    __device__ __forceinline__ StftFrameLoader(const StftFwdArgs& A, unsigned m0)
    {
        const int tid = threadIdx.x;
        x[0] = A.e; x[1] = A.c;
        Tl = (long long)A.T;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned m = m0 + (unsigned)(tid >> 4) + 16u * j;
            aok[j] = m < A.M;
            const unsigned row = aok[j] ? m / A.F : 0u, f = aok[j] ? m - row * A.F : 0u;
            abase[j] = (size_t)row * A.T;
            apos[j] = (long long)f * A.H - A.N / 2 + (tid & 15);
        }
    }
    __device__ __forceinline__ void load(int kt, float (&ra)[NSIG][4]) const
    {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            long long p = apos[j] + kt;
            p = p < 0 ? -p : (p >= Tl ? 2 * (Tl - 1) - p : p);               // reflect, once: N / 2 <= T - 1
#pragma unroll
            for (int s = 0; s < NSIG; ++s) ra[s][j] = aok[j] ? x[s][abase[j] + (size_t)p] : 0.0f;
        }
    }
};

// grid (M / 64 rounded up, BP / 32).  PAIR: both signals and the sums; else `e` alone and mag_out only (the metric).  One block owns
// 64 frames x 32 bins: dft_tile_gemm, then the magnitudes and the block's partial.
template <bool PAIR>
static __global__ __launch_bounds__(WUNET_THREADS) void stft_fwd_kernel(StftFwdArgs A)
{
    constexpr int NSIG = PAIR ? 2 : 1;
    __shared__ __attribute__((aligned(16))) float As[NSIG * WUNET_STFT_FM * WUNET_STFT_AS];
    __shared__ __attribute__((aligned(16))) float Bs[WUNET_STFT_KT * WUNET_STFT_BS];
    __shared__ double red[3 * WUNET_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
    const unsigned m0 = blockIdx.x * WUNET_STFT_FM;
    const int b0 = blockIdx.y * WUNET_STFT_BN;
    wunet_f4 acc[NSIG][2][2];                    // [signal: e, c][re, im][column tile]
    dft_tile_gemm<NSIG>(StftFrameLoader<NSIG>(A, m0), A.basis, A.BP, b0, A.k0, A.k1, As, Bs, acc);
    // ---- epilogue: D[row = 4 lq + r][col = li] of the wave's 16 frames
    double sum[3] = {0.0, 0.0, 0.0};             // (S_c - S_e)^2, S_c^2, |ln S_c - ln S_e|
    const size_t plane = (size_t)A.M * A.BP;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int b = b0 + nt * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned m = m0 + (unsigned)(wave * 16 + lq * 4 + r);
            if (m >= A.M) continue;
            const float re = acc[0][0][nt][r], im = acc[0][1][nt][r];
            const float pe = fmaxf(stft_power(re, im), A.clamp), se = sqrtf(pe);
            if (A.mag_out && b < A.bins) A.mag_out[(size_t)m * A.bins + b] = se;
            if (PAIR) {
                const float pc = fmaxf(stft_power(acc[PAIR ? 1 : 0][0][nt][r], acc[PAIR ? 1 : 0][1][nt][r]), A.clamp), sc = sqrtf(pc);
                if (b < A.bins) {
                    const double d = (double)sc - (double)se;
                    sum[0] += d * d;
                    sum[1] += (double)sc * (double)sc;
                    sum[2] += fabs(0.5 * log((double)pc / (double)pe));     // ln S_c - ln S_e from the powers: one log, no rounding of the roots in it
                }
                if (A.saved) {                                           // (the padding columns too: re = im = 0 there, below the clamp)
                    const size_t o = (size_t)m * A.BP + b;
                    A.saved[o] = re;
                    A.saved[plane + o] = im;
                    A.saved[2 * plane + o] = sc;
                }
            }
        }
    }
    if (PAIR) {
        block_sum<3>(sum, red);
        if (tid == 0) {
            double* o = A.part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
            o[0] = sum[0]; o[1] = sum[1]; o[2] = sum[2];
        }
    }
}

struct StftFinalArgs {
    const double* part[WUNET_STFT_MAX_RES];
    unsigned nparts[WUNET_STFT_MAX_RES];
    double count[WUNET_STFT_MAX_RES];      // rows * F * bins
    int n_res;
    double w_sc, w_mag;
    float* loss;
    double* coefs;                         // [n_res][WUNET_STFT_NCOEF]
};

// ONE block over the table of resolutions: thread t adds partials t, t + 256, ... in that order, block_sum adds the threads (fixed
// order).  a = w_sc / (n_res |S_c - S_e| |S_c|), 0 where S_c == S_e everywhere (the one departure from autograd, which gives NaN);
// b = w_mag / (n_res count).  The loss is accumulated over the resolutions in double and rounded once.
static __global__ __launch_bounds__(WUNET_THREADS) void stft_final_kernel(StftFinalArgs A)
{
    __shared__ double red[3 * WUNET_WAVES];
    const int tid = threadIdx.x;
    double total = 0.0;
    for (int i = 0; i < A.n_res; ++i) {
        double sum[3] = {0.0, 0.0, 0.0};
        for (unsigned p = tid; p < A.nparts[i]; p += WUNET_THREADS) {
            const double* q = A.part[i] + (size_t)p * 3;
            sum[0] += q[0]; sum[1] += q[1]; sum[2] += q[2];
        }
        block_sum<3>(sum, red);
        const double s_d = sum[0];
        const double nd = sqrt(s_d), nc = sqrt(sum[1]);
        const double sc = nd / nc, mag = sum[2] / A.count[i];
        total += A.w_sc * sc + A.w_mag * mag;
        if (tid == 0 && A.coefs) {
            double* o = A.coefs + (size_t)i * WUNET_STFT_NCOEF;
            o[0] = s_d > 0.0 ? A.w_sc / ((double)A.n_res * nd * nc) : 0.0;
            o[1] = A.w_mag / ((double)A.n_res * A.count[i]);
            o[2] = sc;
            o[3] = mag;
        }
    }
    if (tid == 0) *A.loss = (float)(total / (double)A.n_res);
}

struct StftBwdArgs {
    const float* saved;     // [3][M][BP]: re_e, im_e, S_c
    const double* coefs;    // a, b of this resolution
    const float* basis;     // [N][2 BP]
    unsigned M, ktiles;     // ktiles: blocks along the window positions
    int N, BP, bins, k0, k1;
    float clamp;
    float* scratch;         // [M][N], written for k0 <= k < k1
};

// d loss / d (re, im) of one bin from what the forward saved: g = a (S_e - S_c) + b sign(ln S_e - ln S_c) / S_e, times re / S_e and
// im / S_e; nothing where the clamp was active (torch.clamp passes a gradient where P >= clamp)
__device__ __forceinline__ void stft_bin_grad(float re, float im, float sc, float clamp, double ca, double cb, float& dre, float& dim)
{
    const float pe = stft_power(re, im);
    dre = 0.0f; dim = 0.0f;
    if (pe >= clamp) {
        const float se = sqrtf(pe);
        const double inv = 1.0 / (double)se;
        const double sg = se > sc ? 1.0 : (se < sc ? -1.0 : 0.0);
        const double g = (ca * ((double)se - (double)sc) + cb * sg * inv) * inv;
        dre = (float)(g * (double)re);
        dim = (float)(g * (double)im);
    }
}

// What stft_bwd_kernel's loader forms its A from: PLANES saved planes [M][BP] per bin, pad(q) what a row beyond M loads of plane q,
// grad() the bin's (dRe, dIm) from its PLANES values.
struct StftBinGrad {
    static constexpr int PLANES = 3;             // re_e, im_e, S_c
    float clamp;
    double ca, cb;
    __device__ __forceinline__ static float pad(int q) { return q == 2 ? 1.0f : 0.0f; }
    __device__ __forceinline__ void grad(const float (&r)[PLANES], float& dre, float& dim) const { stft_bin_grad(r[0], r[1], r[2], clamp, ca, cb, dre, dim); }
};

// One block of the adjoint GEMM of every loss on this basis (stft_bwd_kernel, cspec_bwd_kernel).  grid ktiles * (M / 64 rounded up), the
// k tiles of one frame tile next to each other (they read the same saved spectra): out[m][k] = sum_b dRe[m][b] cos[k][b] + dIm[m][b] (-sin)[k][b].  K tile = 8 bins:
// Gs[64 frames][8 dRe | 8 dIm] (WUNET_STFT_FM * WUNET_STFT_AS floats), Bt[8 cos | 8 -sin][128 k] (the basis tile transposed on its way
// into LDS; WUNET_STFT_KT * WUNET_STFT_BWS floats).  Bin: see StftBinGrad.
template <class Bin>
__device__ __forceinline__ void dft_adjoint_gemm(const Bin& bin, const float* saved, const float* basis, unsigned M, unsigned ktiles, int N, int BP, int bins,
                                                 int k0, int k1, float* scratch, float* Gs, float* Bt)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
    const int kout0 = k0 + (int)(blockIdx.x % ktiles) * WUNET_STFT_BWN;
    const unsigned m0 = (blockIdx.x / ktiles) * WUNET_STFT_FM;
    const size_t plane = (size_t)M * BP;
    // loader roles.  G: bin tid & 7, frames (tid >> 3) + 32 j.  B: piece = tid + 256 j: window position piece >> 2, quarter piece & 3
    // (cos | -sin, first | second four bins)
    const int gb = tid & 7;
    float rg[2][Bin::PLANES];
    wunet_f4 rb[2];
    const int nb = (bins + 7) & ~7;
#define WUNET_STFT_BLOAD(B0_)                                                                                     \
    do {                                                                                                          \
        _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                           \
            const unsigned m = m0 + (unsigned)(tid >> 3) + 32u * j;                                               \
            const size_t o = (size_t)m * BP + (B0_) + gb;                                                         \
            const bool ok = m < M;                                                                                \
            _Pragma("unroll") for (int q = 0; q < Bin::PLANES; ++q) rg[j][q] = ok ? saved[q * plane + o] : Bin::pad(q); \
            const int piece = tid + WUNET_THREADS * j, k = kout0 + (piece >> 2), qu = piece & 3;                  \
            rb[j] = wunet_sel4(k < k1, wunet_ld4(basis + (size_t)(k < k1 ? k : k0) * 2 * BP + (qu >> 1) * BP + (B0_) + (qu & 1) * 4)); \
        }                                                                                                         \
    } while (0)
    wunet_f4 acc[8];
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) acc[nt] = wunet_f4{0.f, 0.f, 0.f, 0.f};
    WUNET_STFT_BLOAD(0);
    for (int b0 = 0; b0 < nb; b0 += 8) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ml = (tid >> 3) + 32 * j;
            float dre, dim;
            bin.grad(rg[j], dre, dim);
            Gs[ml * WUNET_STFT_AS + gb] = dre;
            Gs[ml * WUNET_STFT_AS + 8 + gb] = dim;
            const int piece = tid + WUNET_THREADS * j, kk = piece >> 2, qu = piece & 3, c = (qu >> 1) * 8 + (qu & 1) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) Bt[(c + e) * WUNET_STFT_BWS + kk] = rb[j][e];
        }
        __syncthreads();
        if (b0 + 8 < nb) WUNET_STFT_BLOAD(b0 + 8);
#pragma unroll
        for (int s4 = 0; s4 < WUNET_STFT_KT / 4; ++s4) {
            const int kk = s4 * 4 + lq;
            const float a = Gs[(wave * 16 + li) * WUNET_STFT_AS + kk];
#pragma unroll
            for (int nt = 0; nt < 8; ++nt) acc[nt] = wunet_mfma16(a, Bt[kk * WUNET_STFT_BWS + nt * 16 + li], acc[nt]);
        }
    }
#undef WUNET_STFT_BLOAD
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) {
        const int k = kout0 + nt * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned m = m0 + (unsigned)(wave * 16 + lq * 4 + r);
            if (m < M && k < k1) scratch[(size_t)m * N + k] = acc[nt][r];
        }
    }
}

static __global__ __launch_bounds__(WUNET_THREADS) void stft_bwd_kernel(StftBwdArgs A)
{
    __shared__ __attribute__((aligned(16))) float Gs[WUNET_STFT_FM * WUNET_STFT_AS];
    __shared__ __attribute__((aligned(16))) float Bt[WUNET_STFT_KT * WUNET_STFT_BWS];
    dft_adjoint_gemm(StftBinGrad{A.clamp, A.coefs[0], A.coefs[1]}, A.saved, A.basis, A.M, A.ktiles, A.N, A.BP, A.bins, A.k0, A.k1, A.scratch, Gs, Bt);
}

struct StftOlaArgs {
    const float* scratch;   // [rows F][N]
    const float* gl;        // grad_loss[0]
    float* g;               // [rows][T]
    size_t T, total;        // total = rows * T
    unsigned F;
    int N, H, k0, k1, accumulate;
};

// every frame f that holds the padded position p inside the window's support, in frame order
__device__ __forceinline__ float stft_ola_at(const StftOlaArgs& A, size_t row, long long p, float sum)
{
    const long long lo = p - A.k1 + 1, hi = p - A.k0;
    if (hi < 0) return sum;
    long long f0 = lo <= 0 ? 0 : (lo + A.H - 1) / A.H, f1 = hi / A.H;
    if (f1 > (long long)A.F - 1) f1 = (long long)A.F - 1;
    for (long long f = f0; f <= f1; ++f) sum += A.scratch[(row * A.F + (size_t)f) * A.N + (size_t)(p - f * A.H)];
    return sum;
}

// A gather: sample t of a row is the padded positions t + N/2, N/2 - t (1 <= t <= N/2, the left reflection) and
// 2 (T - 1) - t + N/2 (T - 1 - N/2 <= t <= T - 2, the right one), summed in that order, times grad_loss; written or accumulated.
static __global__ __launch_bounds__(WUNET_THREADS) void stft_ola_kernel(StftOlaArgs A)
{
    const size_t idx = (size_t)blockIdx.x * WUNET_THREADS + threadIdx.x;
    if (idx >= A.total) return;
    const size_t row = idx / A.T;
    const long long t = (long long)(idx - row * A.T), h = A.N / 2, Tl = (long long)A.T;
    float sum = stft_ola_at(A, row, t + h, 0.0f);
    if (t >= 1 && t <= h) sum = stft_ola_at(A, row, h - t, sum);
    if (t <= Tl - 2 && t >= Tl - 1 - h) sum = stft_ola_at(A, row, 2 * (Tl - 1) - t + h, sum);
    const float v = A.gl[0] * sum;
    A.g[idx] = A.accumulate ? A.g[idx] + v : v;
}
