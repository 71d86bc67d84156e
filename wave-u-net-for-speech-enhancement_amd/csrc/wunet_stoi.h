// STOI per row (include/wunet_hip.h: wunet_stoi_*): Taal et al. 2011 with pystoi's choices for stoi(x, y, fs, extended=False), clean x
// and estimate y, every row of the batch in one launch sequence and no host read - the per-row frame counts live in device memory, the
// grids are sized for the largest possible count and blocks beyond a row's count leave early.
//   stoi_tables_kernel    tables = basis[256][2 BP] (row k = w[k] cos(2 pi k b / 512) for b < BP, then -w[k] sin(..); BP = 224 covers the
//                         bins 7 .. 218 of the third-octave bands) | w[256] = hanning(258)[1:-1] | the resampler's taps, copied
//   stoi_resample_kernel  polyphase FIR to 10 kHz (resample_poly(x, p, q, window = taps)): an output sample reads only the taps of its
//                         phase, staged in LDS; both signals in one launch; double accumulation, one rounding to float
//   stoi_mask_kernel      ONE block per row: energies of the clean row's windowed frames [dB], their maximum, the frames above
//                         maximum - 40 dB as a table kept[row][j] of original frame indices (an exclusive scan) + n_kept[row]
//   stoi_spec_kernel      implicit GEMM [frames][256] x basis on v_mfma_f32_16x16x4_f32 (dft_tile_gemm of wunet_stft.h).  The loader builds
//                         each frame of the silence-free signal from the resampled one and the kept table - w[k] (in the basis) times the
//                         sum of the at most two kept windowed frames over position k - so the overlap-added signal is never written;
//                         the epilogue writes re^2 + im^2 of both signals
//   stoi_segment_kernel   a block owns 64 segments of one row: band magnitudes (the powers of a band added in double, in bin order) of
//                         its 93 frames into LDS, then per (segment, band) the clipped, centred, normalised correlation in double; one
//                         partial per block
//   stoi_final_kernel     one block per row: the partials in block order -> the mean over (segment, band), or 1e-5 below 30 frames
// The loss (include/wunet_hip.h: wunet_stoi_loss_*) runs the same sequence with stoi_spec_kernel<true>, which also keeps re, im of the
// estimate, and stoi_mask_kernel's inverse table; its backward inverts the chain stage by stage, every stage a gather:
//   stoi_loss_final_kernel    ONE block: the rows' double scores added in row order -> -mean, rounded once
//   stoi_segment_bwd_kernel   a block owns 32 frames of one row: band magnitudes of those and of 29 neighbours on each side and the
//                             statistics of the at most 61 segments that touch them into LDS, then per (frame, band) the segments'
//                             contributions in segment order -> gY / Y in double (0 where Y == 0)
//   stoi_spec_bwd_kernel      adjoint GEMM [frames][dRe | dIm] x basis^T -> the frames' gradients [M][256] (the shape of stft_bwd_kernel)
//   stoi_unframe_kernel       one thread per 10 kHz sample: its at most two kept frames x the at most two spectral frames over them
//   stoi_resample_bwd_kernel  the transposed polyphase filter, one thread per input sample, double accumulation
// fp32 operands and MFMA accumulation, every reduction in double and in one fixed order, no atomics: bit-identical run to run.
// ESTOI (extended=True) is this sequence with another segment stage, forward and backward: wunet_estoi.h.
#pragma once
#include "wunet_stft.h"

#define WUNET_STOI_FS 10000          // the rate STOI is defined at
#define WUNET_STOI_N 256             // frame length
#define WUNET_STOI_HOP 128
#define WUNET_STOI_NFFT 512
#define WUNET_STOI_BP 224            // bins 0 .. 223 of the 257: seven tiles of WUNET_STFT_BN
#define WUNET_STOI_BANDS 15
#define WUNET_STOI_SEG 30            // frames per segment
#define WUNET_STOI_SB 64             // segments per block of stoi_segment_kernel
#define WUNET_STOI_MAX_TAPS 4096     // LDS budget of stoi_resample_kernel (16 KiB): 2 L + 1 taps, max(p, q) <= 56
#define WUNET_STOI_RPT 4             // output samples per thread of stoi_resample_kernel
#define WUNET_STOI_FB 32             // frames per block of stoi_segment_bwd_kernel
#define WUNET_STOI_LF 2048           // row scores per LDS chunk of stoi_loss_final_kernel
#define WUNET_STOI_EPS 2.220446049250313e-16
#define WUNET_STOI_TAB_W (WUNET_STOI_N * 2 * WUNET_STOI_BP)              // float offsets inside the tables
#define WUNET_STOI_TAB_TAPS (WUNET_STOI_TAB_W + WUNET_STOI_N)

// first bins of the 15 third-octave bands from 150 Hz at 10 kHz / 512 points, and the end of the last one
__device__ __forceinline__ int stoi_band_edge(int i)
{
    const int e[WUNET_STOI_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};
    return e[i];
}

// grid (N + 1 + ceil(n_taps / 256)): block k < N writes basis row k, block N the window, the rest copy the taps
static __global__ __launch_bounds__(WUNET_THREADS) void stoi_tables_kernel(const float* taps, unsigned n_taps, float* tables)
{
    const int k = blockIdx.x, tid = threadIdx.x;
    double s, c;
    if (k > WUNET_STOI_N) {
        const unsigned i = (unsigned)(k - WUNET_STOI_N - 1) * WUNET_THREADS + tid;
        if (i < n_taps) tables[WUNET_STOI_TAB_TAPS + i] = taps[i];
        return;
    }
    if (k == WUNET_STOI_N) {
        wunet_sincospi_d(2.0 * (double)(tid + 1) / (double)(WUNET_STOI_N + 1), &s, &c);
        tables[WUNET_STOI_TAB_W + tid] = (float)(0.5 - 0.5 * c);
        return;
    }
    wunet_sincospi_d(2.0 * (double)(k + 1) / (double)(WUNET_STOI_N + 1), &s, &c);
    const double w = 0.5 - 0.5 * c;                                      // np.hanning(258)[k + 1]
    for (int col = tid; col < 2 * WUNET_STOI_BP; col += WUNET_THREADS) {
        const int b = col < WUNET_STOI_BP ? col : col - WUNET_STOI_BP;
        const int ph = (k * b) % WUNET_STOI_NFFT;                        // the phase from (k b) mod N in integers
        wunet_sincospi_d(2.0 * (double)ph / (double)WUNET_STOI_NFFT, &s, &c);
        tables[(size_t)k * 2 * WUNET_STOI_BP + col] = (float)(col < WUNET_STOI_BP ? w * c : -(w * s));
    }
}

struct StoiResampleArgs {
    const float* in[2];     // clean, estimate [rows][T]
    const float* taps;      // [2 L + 1], float32
    float* out;             // [2][rows][Tr]
    size_t T, Tr, rows;
    int p, q, L;
};

// grid (Tr / (256 * RPT) rounded up, rows, 2).  y[n] = p sum_t h[t] x[(n q - t) / p] over -L <= t <= L with p | n q - t: with
// c = n q + L, i_hi = c / p and phase = c mod p the terms are h[phase + p j - L] x[i_hi - j], j = 0 .. (2 L - phase) / p, zeros outside x.
static __global__ __launch_bounds__(WUNET_THREADS) void stoi_resample_kernel(StoiResampleArgs A)
{
    __shared__ float hs[WUNET_STOI_MAX_TAPS];
    const int tid = threadIdx.x, ntap = 2 * A.L + 1;
    for (int i = tid; i < ntap; i += WUNET_THREADS) hs[i] = A.taps[i];
    __syncthreads();
    const size_t row = blockIdx.y;
    const float* x = A.in[blockIdx.z] + row * A.T;
    float* y = A.out + ((size_t)blockIdx.z * A.rows + row) * A.Tr;
    const long long Tl = (long long)A.T;
#pragma unroll
    for (int u = 0; u < WUNET_STOI_RPT; ++u) {
        const size_t n = ((size_t)blockIdx.x * WUNET_STOI_RPT + u) * WUNET_THREADS + tid;
        if (n >= A.Tr) continue;
        const long long c = (long long)n * A.q + A.L, ihi = c / A.p;
        const int ph = (int)(c - ihi * A.p);
        long long j0 = ihi - (Tl - 1), j1 = (2 * A.L - ph) / A.p;
        if (j0 < 0) j0 = 0;
        if (j1 > ihi) j1 = ihi;
        double acc = 0.0;
        for (long long j = j0; j <= j1; ++j) acc += (double)hs[ph + A.p * (int)j] * (double)x[ihi - j];
        y[n] = (float)((double)A.p * acc);
    }
}

struct StoiMaskArgs {
    const float* x;         // the clean rows at 10 kHz [rows][Tr]
    const float* w;         // [256]
    size_t Tr;
    unsigned F0;            // frames of a row: starts 0, 128, .. < Tr - 256
    double* energy;         // [rows][F0] scratch
    int* kept;              // [rows][F0]
    int* nk;                // [rows]
    int* inv;               // nullptr or [rows][F0]: original frame -> its index in kept, -1 for a removed one (the loss's backward)
};

// grid (rows).  Pass 1: a wave per frame, E_f = 20 log10(|w x_f| + EPS) with the sum in double (lane l takes samples l, l + 64, ..,
// then a butterfly), and the row's maximum.  Pass 2: thread t owns the frames [t g, (t + 1) g), g = F0 / 256 rounded up; its count of
// kept ones, an exclusive scan of the 256 counts, the indices written in frame order.
static __global__ __launch_bounds__(WUNET_THREADS) void stoi_mask_kernel(StoiMaskArgs A)
{
    __shared__ double wmax[WUNET_WAVES];
    __shared__ unsigned cnt[WUNET_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row = blockIdx.x;
    const float* x = A.x + row * A.Tr;
    double* en = A.energy + row * A.F0;
    float wv[WUNET_STOI_N / 64];
#pragma unroll
    for (int u = 0; u < WUNET_STOI_N / 64; ++u) wv[u] = A.w[lane + 64 * u];
    double emax = -1.0e300;
    for (unsigned f = wave; f < A.F0; f += WUNET_WAVES) {
        const float* xf = x + (size_t)f * WUNET_STOI_HOP;
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < WUNET_STOI_N / 64; ++u) {
            const double v = (double)wv[u] * (double)xf[lane + 64 * u];
            s += v * v;
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) s += wunet_shfl_xor_d(s, m);
        const double e = 20.0 * log10(sqrt(s) + WUNET_STOI_EPS);
        if (lane == 0) en[f] = e;
        emax = e > emax ? e : emax;
    }
    if (lane == 0) wmax[wave] = emax;
    __syncthreads();                                                     // (the energies too: written and read inside this block)
    emax = -1.0e300;
#pragma unroll
    for (int k = 0; k < WUNET_WAVES; ++k) emax = wmax[k] > emax ? wmax[k] : emax;
    const double thr = emax - 40.0;
    const unsigned g = (A.F0 + WUNET_THREADS - 1) / WUNET_THREADS;
    const unsigned f0 = (unsigned)tid * g < A.F0 ? (unsigned)tid * g : A.F0, f1 = f0 + g < A.F0 ? f0 + g : A.F0;
    unsigned n = 0;
    for (unsigned f = f0; f < f1; ++f) n += en[f] > thr ? 1u : 0u;
    cnt[tid] = n;
    __syncthreads();
    unsigned at = 0;
    for (int k = 0; k < tid; ++k) at += cnt[k];
    int* kp = A.kept + row * A.F0;
    for (unsigned f = f0; f < f1; ++f) {
        const bool keep = en[f] > thr;
        if (A.inv) A.inv[row * A.F0 + f] = keep ? (int)at : -1;
        if (keep) kp[at++] = (int)f;
    }
    if (tid == WUNET_THREADS - 1) A.nk[row] = (int)at;
}

struct StoiSpecArgs {
    const float* x[2];      // clean, estimate at 10 kHz [rows][Tr]
    const float* basis;     // [256][2 BP]
    const float* w;         // [256]
    const int* kept;        // [rows][F0]
    const int* nk;          // [rows]
    size_t Tr;
    unsigned M, Fmax, F0;   // Fmax = F0 - 1: the most spectral frames a row can have; M = rows * Fmax
    float* pw;              // [2][M][BP]: re^2 + im^2
    float* reim;            // SAVE: [2][M][BP]: re, im of the estimate
};

// A of stoi_spec_kernel: frame f of the silence-free signal, built from the resampled one and the kept table.  Position k < 128 lies
// in the kept frames f (at k) and f - 1 (at k + 128), k >= 128 in f (at k) and f + 1 (at k - 128); each is windowed once there (ws, the
// window in LDS), and once more by the basis.  Signal 0 = clean, 1 = estimate.
struct StoiFrameLoader {
    const float* x[2];
    const float* ws;
    size_t abase[4];
    int kc[4], kp[4], kn[4];            // the kept frame itself, the one before and the one after it (-1: none)
    __device__ __forceinline__ StoiFrameLoader(const StoiSpecArgs& A, unsigned m0, const float* ws_) : ws(ws_)
    {
        const int tid = threadIdx.x;
        x[0] = A.x[0]; x[1] = A.x[1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned m = m0 + (unsigned)(tid >> 4) + 16u * j;
            const unsigned row = m < A.M ? m / A.Fmax : 0u, f = m - row * A.Fmax;
            const bool ok = m < A.M && (int)f < A.nk[row] - 1;
            const int* kr = A.kept + (size_t)row * A.F0;
            abase[j] = (size_t)row * A.Tr;
            kc[j] = ok ? kr[f] : -1;
            kp[j] = ok && f > 0 ? kr[f - 1] : -1;
            kn[j] = ok ? kr[f + 1] : -1;
        }
    }
    __device__ __forceinline__ void load(int kt, float (&ra)[2][4]) const
    {
        const int k = kt + ((int)threadIdx.x & 15), ko = k < WUNET_STOI_HOP ? k + WUNET_STOI_HOP : k - WUNET_STOI_HOP;
        const float w = ws[k], wo = ws[ko];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int other = k < WUNET_STOI_HOP ? kp[j] : kn[j];
            const size_t o1 = abase[j] + (size_t)(kc[j] < 0 ? 0 : kc[j]) * WUNET_STOI_HOP + k;
            const size_t o2 = abase[j] + (size_t)(other < 0 ? 0 : other) * WUNET_STOI_HOP + ko;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const float v1 = kc[j] < 0 ? 0.0f : w * x[s][o1];
                const float v2 = other < 0 ? 0.0f : wo * x[s][o2];
                ra[s][j] = v1 + v2;
            }
        }
    }
};

// grid (M / 64 rounded up, BP / 32).  Frame m = row * Fmax + f is live for f < n_kept[row] - 1.  One block owns 64 frames x 32 bins of
// both signals: dft_tile_gemm (wunet_stft.h) over the 256 window positions, then the powers.  SAVE (the loss): re and im of the estimate
// as well - the same accumulators, the same powers.
template <bool SAVE>
static __global__ __launch_bounds__(WUNET_THREADS) void stoi_spec_kernel(StoiSpecArgs A)
{
    __shared__ __attribute__((aligned(16))) float As[2 * WUNET_STFT_FM * WUNET_STFT_AS];
    __shared__ __attribute__((aligned(16))) float Bs[WUNET_STFT_KT * WUNET_STFT_BS];
    __shared__ float ws[WUNET_STOI_N];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
    const unsigned m0 = blockIdx.x * WUNET_STFT_FM;
    const int b0 = blockIdx.y * WUNET_STFT_BN;
    {   // leave when none of the block's frames is live (the same answer in every thread)
        const unsigned mlast = m0 + WUNET_STFT_FM - 1 < A.M - 1 ? m0 + WUNET_STFT_FM - 1 : A.M - 1;
        bool any = false;
        for (unsigned r = m0 / A.Fmax; r <= mlast / A.Fmax; ++r) {
            const int live = A.nk[r] - 1;
            const unsigned lo = r * A.Fmax > m0 ? r * A.Fmax : m0;
            any = any || (live > 0 && lo < r * A.Fmax + (unsigned)live);
        }
        if (!any) return;
    }
    ws[tid] = A.w[tid];
    const StoiFrameLoader loader(A, m0, ws);
    __syncthreads();                                                     // ws
    wunet_f4 acc[2][2][2];               // [signal][re, im][column tile]
    dft_tile_gemm<2>(loader, A.basis, WUNET_STOI_BP, b0, 0, WUNET_STOI_N, As, Bs, acc);
    // ---- epilogue: D[row = 4 lq + r][col = li] of the wave's 16 frames (a dead frame of a live block: zeros, never read)
    const size_t plane = (size_t)A.M * WUNET_STOI_BP;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int b = b0 + nt * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned m = m0 + (unsigned)(wave * 16 + lq * 4 + r);
            if (m >= A.M) continue;
            const size_t o = (size_t)m * WUNET_STOI_BP + b;
            A.pw[o] = stft_power(acc[0][0][nt][r], acc[0][1][nt][r]);
            A.pw[plane + o] = stft_power(acc[1][0][nt][r], acc[1][1][nt][r]);
            if (SAVE) {
                A.reim[o] = acc[1][0][nt][r];
                A.reim[plane + o] = acc[1][1][nt][r];
            }
        }
    }
}

struct StoiSegArgs {
    const float* pw;        // [2][M][BP]
    const int* nk;          // [rows]
    unsigned M, Fmax, nblk; // nblk = (Fmax - 29) / 64 rounded up: the grid's x
    double clip;            // 1 + 10^(15 / 20)
    double* part;           // [rows][nblk]
};

// frames of a row -> segments: 0 below 30 frames
__device__ __forceinline__ int stoi_segments(int n_kept)
{
    const int fs = n_kept - 1;
    return fs >= WUNET_STOI_SEG ? fs - WUNET_STOI_SEG + 1 : 0;
}

// grid (nblk, rows).  With X, Y the 30 band magnitudes of a segment: alpha = |X| / (|Y| + EPS), Y' = min(alpha Y, clip X), both
// centred, each divided by (its norm + EPS), d = sum X Y' - all of it in double; a thread adds the d of its (segment, band) items
// in index order, block_sum the threads.
static __global__ __launch_bounds__(WUNET_THREADS) void stoi_segment_kernel(StoiSegArgs A)
{
    __shared__ double tb[2 * (WUNET_STOI_SB + WUNET_STOI_SEG - 1) * WUNET_STOI_BANDS];
    __shared__ double red[WUNET_WAVES];
    const int tid = threadIdx.x;
    const size_t row = blockIdx.y;
    const int nseg = stoi_segments(A.nk[row]), s0 = (int)blockIdx.x * WUNET_STOI_SB;
    if (s0 >= nseg) return;
    const int ns = nseg - s0 < WUNET_STOI_SB ? nseg - s0 : WUNET_STOI_SB, nf = ns + WUNET_STOI_SEG - 1;
    const size_t plane = (size_t)A.M * WUNET_STOI_BP;
    constexpr int TBS = (WUNET_STOI_SB + WUNET_STOI_SEG - 1) * WUNET_STOI_BANDS;
    for (int i = tid; i < 2 * nf * WUNET_STOI_BANDS; i += WUNET_THREADS) {
        const int sig = i / (nf * WUNET_STOI_BANDS), fb = i - sig * nf * WUNET_STOI_BANDS, fr = fb / WUNET_STOI_BANDS, band = fb - fr * WUNET_STOI_BANDS;
        const float* p = A.pw + sig * plane + (row * A.Fmax + (size_t)(s0 + fr)) * WUNET_STOI_BP;
        double s = 0.0;
        for (int b = stoi_band_edge(band); b < stoi_band_edge(band + 1); ++b) s += (double)p[b];
        tb[sig * TBS + fb] = sqrt(s);
    }
    __syncthreads();
    double dsum[1] = {0.0};
    for (int i = tid; i < ns * WUNET_STOI_BANDS; i += WUNET_THREADS) {
        const double* xs = tb + i;                                       // (segment i / 15, band i % 15): frame n at + 15 n
        const double* ys = tb + TBS + i;
        double sx2 = 0.0, sy2 = 0.0, sx = 0.0;
#pragma unroll
        for (int n = 0; n < WUNET_STOI_SEG; ++n) {
            const double x = xs[n * WUNET_STOI_BANDS], y = ys[n * WUNET_STOI_BANDS];
            sx2 += x * x; sy2 += y * y; sx += x;
        }
        const double alpha = sqrt(sx2) / (sqrt(sy2) + WUNET_STOI_EPS);
        double sy = 0.0;
#pragma unroll
        for (int n = 0; n < WUNET_STOI_SEG; ++n) {
            const double x = xs[n * WUNET_STOI_BANDS], y = alpha * ys[n * WUNET_STOI_BANDS], c = x * A.clip;
            sy += y < c ? y : c;
        }
        const double mx = sx / WUNET_STOI_SEG, my = sy / WUNET_STOI_SEG;
        double cxx = 0.0, cyy = 0.0, cxy = 0.0;
#pragma unroll
        for (int n = 0; n < WUNET_STOI_SEG; ++n) {
            const double x = xs[n * WUNET_STOI_BANDS], y = alpha * ys[n * WUNET_STOI_BANDS], c = x * A.clip;
            const double xc = x - mx, yc = (y < c ? y : c) - my;
            cxx += xc * xc; cyy += yc * yc; cxy += xc * yc;
        }
        dsum[0] += cxy / ((sqrt(cxx) + WUNET_STOI_EPS) * (sqrt(cyy) + WUNET_STOI_EPS));
    }
    block_sum<1>(dsum, red);
    if (tid == 0) A.part[row * A.nblk + blockIdx.x] = dsum[0];
}

// grid (rows).  nk == nullptr: rows too short for one frame.  Thread t adds partials t, t + 256, .. in that order.
// out / score (either may be nullptr): the row's score rounded to float / as the double it was computed in.
static __global__ __launch_bounds__(WUNET_THREADS) void stoi_final_kernel(const double* part, const int* nk, unsigned nblk, float* out, int* frames,
                                                                         double* score)
{
    __shared__ double red[WUNET_WAVES];
    const int tid = threadIdx.x;
    const size_t row = blockIdx.x;
    const int n_kept = nk ? nk[row] : 0, nseg = stoi_segments(n_kept);
    const int nb = (nseg + WUNET_STOI_SB - 1) / WUNET_STOI_SB;
    double s[1] = {0.0};
    for (int b = tid; b < nb; b += WUNET_THREADS) s[0] += part[row * nblk + b];
    block_sum<1>(s, red);
    if (tid == 0) {
        const double v = s[0] / ((double)nseg * WUNET_STOI_BANDS);
        if (out) out[row] = nseg > 0 ? (float)v : 1.0e-5f;
        if (score) score[row] = nseg > 0 ? v : 1.0e-5;
        if (frames) frames[row] = n_kept > 0 ? n_kept - 1 : 0;
    }
}

// ---------------------------------------------------------------------------- the loss: -mean of the rows' scores, and its backward
// ONE block.  The scores pass through LDS in chunks of WUNET_STOI_LF and thread 0 adds them in row order.
static __global__ __launch_bounds__(WUNET_THREADS) void stoi_loss_final_kernel(const double* score, unsigned rows, float* loss)
{
    __shared__ double sv[WUNET_STOI_LF];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (unsigned r0 = 0; r0 < rows; r0 += WUNET_STOI_LF) {
        const unsigned n = rows - r0 < WUNET_STOI_LF ? rows - r0 : WUNET_STOI_LF;
        __syncthreads();                                                 // the previous chunk is read
        for (unsigned i = tid; i < n; i += WUNET_THREADS) sv[i] = score[r0 + i];
        __syncthreads();
        if (tid == 0)
            for (unsigned i = 0; i < n; ++i) s += sv[i];
    }
    if (tid == 0) *loss = (float)(-s / (double)rows);
}

struct StoiSegBwdArgs {
    const float* pw;        // [2][M][BP], as the forward left it
    const int* nk;          // [rows]
    const float* gl;        // grad_loss[0]
    unsigned M, Fmax;
    double clip, inv_rows;  // 1 / rows
    double* gr;             // [M][15]: d loss / d Y divided by Y, written for the frames of the rows that have a segment
};

// grid (Fmax / 32 rounded up, rows).  Segment (m, band) with X, Y its 30 magnitudes, alpha, Y' = min(alpha Y, clip X), the centred xc, yc,
// Dx = |xc| + EPS, N = |yc|, D = N + EPS, c = sum xc yc / Dx, K = c / (D^2 N):  d d / d Y'_n = xc_n / (D Dx) - K yc_n =: h_n (its mean over n
// is 0: the centring passes it unchanged), which reaches Y_n through alpha Y_n where alpha Y_n < clip X_n (u_n = 1) and through alpha
// itself: d d / d Y_n = u_n alpha h_n - P3 Y_n, P3 = alpha S / ((|Y| + EPS) |Y|), S = sum u_n h_n Y_n.  Five numbers per segment and band
// in LDS - alpha, P1 = alpha / (D Dx), P2 = alpha^2 K, Q = alpha (K my - mx / (D Dx)), P3 - give
// u_n (P1 X_n - P2 Y_n + Q) - P3 Y_n.  K = 0 where N == 0 and P3 = 0 where |Y| == 0 (autograd: NaN).  Frame f adds its segments
// max(0, f - 29) .. min(f, n_seg - 1) in that order; times -grad_loss / (rows 15 n_seg); divided by Y, 0 where Y == 0.
static __global__ __launch_bounds__(WUNET_THREADS) void stoi_segment_bwd_kernel(StoiSegBwdArgs A)
{
    constexpr int NS = WUNET_STOI_FB + WUNET_STOI_SEG - 1, NF = NS + WUNET_STOI_SEG - 1;    // 61 segments over 90 frames at the most
    constexpr int TBS = NF * WUNET_STOI_BANDS, SCS = NS * WUNET_STOI_BANDS;
    __shared__ double tb[2 * TBS];
    __shared__ double sc[5 * SCS];
    const int tid = threadIdx.x;
    const size_t row = blockIdx.y;
    const int nfr = A.nk[row] - 1, nseg = stoi_segments(A.nk[row]), f0 = (int)blockIdx.x * WUNET_STOI_FB;
    if (nseg == 0 || f0 >= nfr) return;
    const int f1 = f0 + WUNET_STOI_FB < nfr ? f0 + WUNET_STOI_FB : nfr;                      // the block's frames [f0, f1)
    const int m0 = f0 - (WUNET_STOI_SEG - 1) > 0 ? f0 - (WUNET_STOI_SEG - 1) : 0, m1 = f1 - 1 < nseg - 1 ? f1 - 1 : nseg - 1;
    const int ns = m1 - m0 + 1, nf = ns + WUNET_STOI_SEG - 1;                                // segments m0 .. m1 over frames m0 .. m1 + 29
    const size_t plane = (size_t)A.M * WUNET_STOI_BP;
    for (int i = tid; i < 2 * nf * WUNET_STOI_BANDS; i += WUNET_THREADS) {                   // (the forward's sums: the same bits)
        const int sig = i / (nf * WUNET_STOI_BANDS), fb = i - sig * nf * WUNET_STOI_BANDS, fr = fb / WUNET_STOI_BANDS, band = fb - fr * WUNET_STOI_BANDS;
        const float* p = A.pw + sig * plane + (row * A.Fmax + (size_t)(m0 + fr)) * WUNET_STOI_BP;
        double s = 0.0;
        for (int b = stoi_band_edge(band); b < stoi_band_edge(band + 1); ++b) s += (double)p[b];
        tb[sig * TBS + fb] = sqrt(s);
    }
    __syncthreads();
    for (int i = tid; i < ns * WUNET_STOI_BANDS; i += WUNET_THREADS) {
        const double* xs = tb + i;                                       // (segment m0 + i / 15, band i % 15): frame n at + 15 n
        const double* ys = tb + TBS + i;
        double sx2 = 0.0, sy2 = 0.0, sx = 0.0;
#pragma unroll
        for (int n = 0; n < WUNET_STOI_SEG; ++n) {
            const double x = xs[n * WUNET_STOI_BANDS], y = ys[n * WUNET_STOI_BANDS];
            sx2 += x * x; sy2 += y * y; sx += x;
        }
        const double ny = sqrt(sy2), alpha = sqrt(sx2) / (ny + WUNET_STOI_EPS);
        double sy = 0.0;
#pragma unroll
        for (int n = 0; n < WUNET_STOI_SEG; ++n) {
            const double x = xs[n * WUNET_STOI_BANDS], y = alpha * ys[n * WUNET_STOI_BANDS], c = x * A.clip;
            sy += y < c ? y : c;
        }
        const double mx = sx / WUNET_STOI_SEG, my = sy / WUNET_STOI_SEG;
        double cxx = 0.0, cyy = 0.0, cxy = 0.0;
#pragma unroll
        for (int n = 0; n < WUNET_STOI_SEG; ++n) {
            const double x = xs[n * WUNET_STOI_BANDS], y = alpha * ys[n * WUNET_STOI_BANDS], c = x * A.clip;
            const double xc = x - mx, yc = (y < c ? y : c) - my;
            cxx += xc * xc; cyy += yc * yc; cxy += xc * yc;
        }
        const double dx = sqrt(cxx) + WUNET_STOI_EPS, nyc = sqrt(cyy), d = nyc + WUNET_STOI_EPS;
        const double a1 = 1.0 / (d * dx), k = nyc > 0.0 ? cxy / (dx * d * d * nyc) : 0.0;
        double s = 0.0;
#pragma unroll
        for (int n = 0; n < WUNET_STOI_SEG; ++n) {
            const double x = xs[n * WUNET_STOI_BANDS], y0 = ys[n * WUNET_STOI_BANDS], y = alpha * y0, c = x * A.clip;
            if (y < c) s += (a1 * (x - mx) - k * (y - my)) * y0;
        }
        sc[i] = alpha;
        sc[SCS + i] = alpha * a1;
        sc[2 * SCS + i] = alpha * alpha * k;
        sc[3 * SCS + i] = alpha * (k * my - a1 * mx);
        sc[4 * SCS + i] = ny > 0.0 ? alpha * s / ((ny + WUNET_STOI_EPS) * ny) : 0.0;
    }
    __syncthreads();
    const double scale = -(double)A.gl[0] * A.inv_rows / ((double)nseg * WUNET_STOI_BANDS);
    for (int i = tid; i < (f1 - f0) * WUNET_STOI_BANDS; i += WUNET_THREADS) {
        const int fl = i / WUNET_STOI_BANDS, band = i - fl * WUNET_STOI_BANDS, f = f0 + fl;
        const double x = tb[(f - m0) * WUNET_STOI_BANDS + band], y = tb[TBS + (f - m0) * WUNET_STOI_BANDS + band], c = x * A.clip;
        const int lo = f - (WUNET_STOI_SEG - 1) > 0 ? f - (WUNET_STOI_SEG - 1) : 0, hi = f < nseg - 1 ? f : nseg - 1;
        double g = 0.0;
        for (int m = lo; m <= hi; ++m) {
            const int j = (m - m0) * WUNET_STOI_BANDS + band;
            const double through = sc[j] * y < c ? sc[SCS + j] * x - sc[2 * SCS + j] * y + sc[3 * SCS + j] : 0.0;
            g += through - sc[4 * SCS + j] * y;
        }
        A.gr[(row * A.Fmax + (size_t)f) * WUNET_STOI_BANDS + band] = y > 0.0 ? g * scale / y : 0.0;
    }
}

struct StoiSpecBwdArgs {
    const float* reim;      // [2][M][BP]: re, im of the estimate
    const double* gr;       // [M][15]
    const float* basis;     // [256][2 BP]
    const int* nk;          // [rows]
    unsigned M, Fmax;
    float* fg;              // [M][256]: d loss / d (frame of the silence-free signal), written for the live blocks
};

// the frames of a row that the backward visits: all of its spectral frames, or none where it has no segment
__device__ __forceinline__ int stoi_bwd_frames(int n_kept) { return stoi_segments(n_kept) > 0 ? n_kept - 1 : 0; }

// grid 2 * (M / 64 rounded up), the two halves of the window of one frame tile next to each other:
// fg[m][k] = sum_b dRe[m][b] cos[k][b] + dIm[m][b] (-sin)[k][b] with dRe = (gY / Y) re, dIm = (gY / Y) im, 0 outside the bands' bins 7 .. 218
// and for a dead frame.  stft_bwd_kernel's shape: K tile = 8 bins, Gs[64 frames][8 dRe | 8 dIm], Bt[8 cos | 8 -sin][128 k] (the basis
// tile transposed on its way into LDS); 28 K tiles, no tail.  A block without a live frame leaves at once.
static __global__ __launch_bounds__(WUNET_THREADS) void stoi_spec_bwd_kernel(StoiSpecBwdArgs A)
{
    __shared__ __attribute__((aligned(16))) float Gs[WUNET_STFT_FM * WUNET_STFT_AS];
    __shared__ __attribute__((aligned(16))) float Bt[WUNET_STFT_KT * WUNET_STFT_BWS];
    __shared__ signed char band_of[WUNET_STOI_BP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
    const int kout0 = (int)(blockIdx.x & 1) * WUNET_STFT_BWN;
    const unsigned m0 = (blockIdx.x >> 1) * WUNET_STFT_FM;
    {   // (the same answer in every thread)
        const unsigned mlast = m0 + WUNET_STFT_FM - 1 < A.M - 1 ? m0 + WUNET_STFT_FM - 1 : A.M - 1;
        bool any = false;
        for (unsigned r = m0 / A.Fmax; r <= mlast / A.Fmax; ++r) {
            const int live = stoi_bwd_frames(A.nk[r]);
            const unsigned lo = r * A.Fmax > m0 ? r * A.Fmax : m0;
            any = any || (live > 0 && lo < r * A.Fmax + (unsigned)live);
        }
        if (!any) return;
    }
    if (tid < WUNET_STOI_BP) {
        int band = -1;
        for (int i = 0; i < WUNET_STOI_BANDS; ++i)
            if (tid >= stoi_band_edge(i) && tid < stoi_band_edge(i + 1)) band = i;
        band_of[tid] = (signed char)band;
    }
    const size_t plane = (size_t)A.M * WUNET_STOI_BP;
    // loader roles.  G: bin tid & 7, frames (tid >> 3) + 32 j.  B: piece = tid + 256 j: window position piece >> 2, quarter piece & 3
    // (cos | -sin, first | second four bins)
    const int gb = tid & 7;
    size_t go[2];
    bool gok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const unsigned m = m0 + (unsigned)(tid >> 3) + 32u * j;
        const unsigned row = m < A.M ? m / A.Fmax : 0u;
        gok[j] = m < A.M && (int)(m - row * A.Fmax) < stoi_bwd_frames(A.nk[row]);
        go[j] = gok[j] ? (size_t)m : 0;
    }
    __syncthreads();                                                     // band_of
    float rg[2][2];
    double rr[2];
    wunet_f4 rb[2];
#define WUNET_STOI_BLOAD(B0_)                                                                                     \
    do {                                                                                                          \
        const int band = band_of[(B0_) + gb];                                                                     \
        _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                           \
            const size_t o = go[j] * WUNET_STOI_BP + (B0_) + gb;                                                  \
            const bool ok = gok[j] && band >= 0;                                                                  \
            rg[j][0] = ok ? A.reim[o] : 0.0f;                                                                     \
            rg[j][1] = ok ? A.reim[plane + o] : 0.0f;                                                             \
            rr[j] = ok ? A.gr[go[j] * WUNET_STOI_BANDS + band] : 0.0;                                             \
            const int piece = tid + WUNET_THREADS * j, k = kout0 + (piece >> 2), qu = piece & 3;                  \
            rb[j] = wunet_ld4(A.basis + (size_t)k * 2 * WUNET_STOI_BP + (qu >> 1) * WUNET_STOI_BP + (B0_) + (qu & 1) * 4); \
        }                                                                                                         \
    } while (0)
    wunet_f4 acc[8];
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) acc[nt] = wunet_f4{0.f, 0.f, 0.f, 0.f};
    WUNET_STOI_BLOAD(0);
    for (int b0 = 0; b0 < WUNET_STOI_BP; b0 += 8) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ml = (tid >> 3) + 32 * j;
            Gs[ml * WUNET_STFT_AS + gb] = (float)(rr[j] * (double)rg[j][0]);
            Gs[ml * WUNET_STFT_AS + 8 + gb] = (float)(rr[j] * (double)rg[j][1]);
            const int piece = tid + WUNET_THREADS * j, kk = piece >> 2, qu = piece & 3, c = (qu >> 1) * 8 + (qu & 1) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) Bt[(c + e) * WUNET_STFT_BWS + kk] = rb[j][e];
        }
        __syncthreads();
        if (b0 + 8 < WUNET_STOI_BP) WUNET_STOI_BLOAD(b0 + 8);
#pragma unroll
        for (int s4 = 0; s4 < WUNET_STFT_KT / 4; ++s4) {
            const int kk = s4 * 4 + lq;
            const float a = Gs[(wave * 16 + li) * WUNET_STFT_AS + kk];
#pragma unroll
            for (int nt = 0; nt < 8; ++nt) acc[nt] = wunet_mfma16(a, Bt[kk * WUNET_STFT_BWS + nt * 16 + li], acc[nt]);
        }
    }
#undef WUNET_STOI_BLOAD
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) {
        const int k = kout0 + nt * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned m = m0 + (unsigned)(wave * 16 + lq * 4 + r);
            if (m < A.M) A.fg[(size_t)m * WUNET_STOI_N + k] = acc[nt][r];
        }
    }
}

struct StoiUnframeArgs {
    const float* fg;        // [M][256]
    const float* w;         // [256]
    const int* inv;         // [rows][F0]
    const int* nk;          // [rows]; nullptr: no row has a segment
    float* g;               // [rows][Tr]: the gradient at 10 kHz
    size_t Tr, total;       // total = rows * Tr
    unsigned Fmax, F0;
};

// One thread per 10 kHz sample t.  The kept frame with index i that holds t at k puts w[k] y[t] at position p = 128 i + k of the
// silence-free signal, and spectral frame f < n_kept - 1 reads p at p - 128 f: g[t] = sum over the original frames j = t / 128 - 1,
// t / 128 that are kept (i = inv[j]) of w[k] (fg[p / 128 - 1][..] + fg[p / 128][..]), in that order, in double, rounded once.  A sample in
// no kept frame, past the last frame, or of a row without a segment gets an exact 0.
static __global__ __launch_bounds__(WUNET_THREADS) void stoi_unframe_kernel(StoiUnframeArgs A)
{
    const size_t idx = (size_t)blockIdx.x * WUNET_THREADS + threadIdx.x;
    if (idx >= A.total) return;
    const size_t row = idx / A.Tr;
    const long long t = (long long)(idx - row * A.Tr);
    const int nfr = A.nk ? stoi_bwd_frames(A.nk[row]) : 0;
    double sum = 0.0;
    if (nfr > 0) {
        const long long j1 = t / WUNET_STOI_HOP;
        for (long long j = j1 > 0 ? j1 - 1 : 0; j <= j1 && j < (long long)A.F0; ++j) {
            const int i = A.inv[row * A.F0 + (size_t)j];
            if (i < 0) continue;
            const int k = (int)(t - j * WUNET_STOI_HOP);
            const long long p = (long long)i * WUNET_STOI_HOP + k, fp = p / WUNET_STOI_HOP;
            double s = 0.0;
            for (long long f = fp > 0 ? fp - 1 : 0; f <= fp && f < (long long)nfr; ++f)
                s += (double)A.fg[(row * A.Fmax + (size_t)f) * WUNET_STOI_N + (size_t)(p - f * WUNET_STOI_HOP)];
            sum += (double)A.w[k] * s;
        }
    }
    A.g[idx] = (float)sum;
}

struct StoiResampleBwdArgs {
    const float* gy;        // [rows][Tr]: the gradient at 10 kHz
    const float* taps;      // [2 L + 1]
    float* gx;              // [rows][T]
    size_t T, Tr;
    int p, q, L;
};

// grid (T / (256 * RPT) rounded up, rows).  The transposed filter: gx[i] = p sum_n h[n q + L - p i] gy[n] over the n with
// 0 <= n q + L - p i <= 2 L and n < Tr, in the order of n.
static __global__ __launch_bounds__(WUNET_THREADS) void stoi_resample_bwd_kernel(StoiResampleBwdArgs A)
{
    __shared__ float hs[WUNET_STOI_MAX_TAPS];
    const int tid = threadIdx.x, ntap = 2 * A.L + 1;
    for (int i = tid; i < ntap; i += WUNET_THREADS) hs[i] = A.taps[i];
    __syncthreads();
    const size_t row = blockIdx.y;
    const float* gy = A.gy + row * A.Tr;
    float* gx = A.gx + row * A.T;
#pragma unroll
    for (int u = 0; u < WUNET_STOI_RPT; ++u) {
        const size_t i = ((size_t)blockIdx.x * WUNET_STOI_RPT + u) * WUNET_THREADS + tid;
        if (i >= A.T) continue;
        const long long c = (long long)i * A.p - A.L;                    // n q >= c
        long long n0 = c > 0 ? (c + A.q - 1) / A.q : 0, n1 = (c + 2 * A.L) / A.q;
        if (n1 > (long long)A.Tr - 1) n1 = (long long)A.Tr - 1;
        double acc = 0.0;
        for (long long n = n0; n <= n1; ++n) acc += (double)hs[(int)(n * A.q - c)] * (double)gy[n];
        gx[i] = (float)((double)A.p * acc);
    }
}
