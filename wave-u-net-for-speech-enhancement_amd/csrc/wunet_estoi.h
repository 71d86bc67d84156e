// ESTOI per row (include/wunet_hip.h: wunet_estoi_*): Jensen & Taal 2016 with pystoi's choices for stoi(x, y, fs, extended=True).  Everything
// up to the band powers is the STOI sequence of wunet_stoi.h, unchanged; only the segment stage differs, forward and backward.  With
// X[n][j], Y[n][j] the band magnitudes of the 30 frames n and 15 bands j of a segment, for X and, separately, for Y:
//   rows     per band j over the 30 frames: minus the mean, times r = 1 / (norm + EPS)          -> xr, yr
//   columns  per frame n over the 15 bands of xr / yr: minus the mean, over (norm + EPS)         -> x~, y~
//   d = (1 / 30) sum_n sum_j x~ y~; the row's score is the mean of d over its segments.
// pystoi adds EPS * randn to the block before each normalisation, only to avoid 0 / 0; nothing is added here and EPS stands in the
// two denominators instead (a difference at the 1e-15 level on any non-degenerate input).  A band row or a frame column whose centred
// norm is exactly 0 normalises to zeros and passes no gradient (autograd: NaN).
//   estoi_segment_kernel      takes stoi_segment_kernel's place: a block owns 64 segments of one row, the same band magnitudes in LDS
//                             (the same sums in bin order: the same bits), then per (segment, band) the row statistics and, behind a
//                             barrier, per (segment, frame) the column statistics and the frame's share of d; one partial per block
//                             for stoi_final_kernel / stoi_loss_final_kernel
//   estoi_segment_bwd_kernel  a block owns 16 segments of one row and leaves each segment's 30 x 15 block d d / d Y in scratch
//   estoi_gather_kernel       one thread per (frame, band): the blocks of its at most 30 segments added in segment order -> the gr[M][15]
//                             that stoi_segment_bwd_kernel writes, so stoi_spec_bwd_kernel and the stages behind it run unchanged
// Two launches for the backward: the per-segment state is 6 x 15 row numbers and 4 x 30 column numbers, which for the 61 segments that
// touch a 32-frame tile is 100 KiB of LDS and one block per CU, every block repeating the statistics of its neighbours' segments.
// Per segment blocks do each statistic once, keep 37 KiB a block, and the gather reads 30 x 15 doubles a segment (11 MB at 64 x 16384,
// 16 kHz) once, coalesced.  Doubles throughout, gathers only, one fixed order, no atomics: bit-identical run to run.
#pragma once
#include "wunet_stoi.h"

#define WUNET_ESTOI_SGB 16           // segments per block of estoi_segment_bwd_kernel
#define WUNET_ESTOI_BLK (WUNET_STOI_SEG * WUNET_STOI_BANDS)             // doubles of a segment's gradient block

// the magnitude of one band of one frame, p = the frame's powers [BP]: stoi_segment_kernel's sum, the same bits
__device__ __forceinline__ double estoi_band(const float* p, int band)
{
    double s = 0.0;
    for (int b = stoi_band_edge(band); b < stoi_band_edge(band + 1); ++b) s += (double)p[b];
    return sqrt(s);
}

// band magnitudes of the frames [f0, f0 + nf) of row `row`, both signals: tb[sig * tbs + frame * 15 + band]
__device__ __forceinline__ void estoi_load_bands(const float* pw, size_t plane, size_t row, unsigned Fmax, int f0, int nf, double* tb, int tbs)
{
    for (int i = threadIdx.x; i < 2 * nf * WUNET_STOI_BANDS; i += WUNET_THREADS) {
        const int sig = i / (nf * WUNET_STOI_BANDS), fb = i - sig * nf * WUNET_STOI_BANDS, fr = fb / WUNET_STOI_BANDS, band = fb - fr * WUNET_STOI_BANDS;
        tb[sig * tbs + fb] = estoi_band(pw + sig * plane + (row * Fmax + (size_t)(f0 + fr)) * WUNET_STOI_BP, band);
    }
}

// one band of one segment, v = its 30 magnitudes at stride 15: mean, norm of the centred row, r = 1 / (norm + EPS) (0 where the norm is 0)
struct EstoiRow { double m, n, r; };
__device__ __forceinline__ EstoiRow estoi_row(const double* v)
{
    EstoiRow o;
    double s = 0.0, c = 0.0;
#pragma unroll
    for (int n = 0; n < WUNET_STOI_SEG; ++n) s += v[n * WUNET_STOI_BANDS];
    o.m = s / WUNET_STOI_SEG;
#pragma unroll
    for (int n = 0; n < WUNET_STOI_SEG; ++n) {
        const double d = v[n * WUNET_STOI_BANDS] - o.m;
        c += d * d;
    }
    o.n = sqrt(c);
    o.r = o.n > 0.0 ? 1.0 / (o.n + WUNET_STOI_EPS) : 0.0;
    return o;
}

// one frame of one segment, xf / yf = its 15 magnitudes, mx / rx / my / ry = the segment's row statistics [15]: the means of the
// row-normalised columns, the norms of the centred ones and their dot product
struct EstoiCol { double cx, cy, nx, ny, sxy; };
__device__ __forceinline__ EstoiCol estoi_col(const double* xf, const double* yf, const double* mx, const double* rx, const double* my, const double* ry)
{
    EstoiCol o;
    double xr[WUNET_STOI_BANDS], yr[WUNET_STOI_BANDS], sx = 0.0, sy = 0.0;
#pragma unroll
    for (int j = 0; j < WUNET_STOI_BANDS; ++j) {
        xr[j] = (xf[j] - mx[j]) * rx[j];
        yr[j] = (yf[j] - my[j]) * ry[j];
        sx += xr[j]; sy += yr[j];
    }
    o.cx = sx / WUNET_STOI_BANDS; o.cy = sy / WUNET_STOI_BANDS;
    double sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
    for (int j = 0; j < WUNET_STOI_BANDS; ++j) {
        const double xc = xr[j] - o.cx, yc = yr[j] - o.cy;
        sxx += xc * xc; syy += yc * yc; sxy += xc * yc;
    }
    o.nx = sqrt(sxx); o.ny = sqrt(syy); o.sxy = sxy;
    return o;
}

// grid (nblk, rows), StoiSegArgs without its clip.  LDS: the magnitudes 2 x 93 x 15 doubles (21.8 KiB) + four row statistics per
// (segment, band) 4 x 64 x 15 doubles (30 KiB) = 51.8 KiB, under the 64 KiB of a static allocation and three blocks to a CU; 64 segments
// a block is also what stoi_final_kernel divides `part` by.  A thread adds the shares of its (segment, frame) items in index order,
// block_sum the threads; times 1 / 2, exact, because stoi_final_kernel divides by 15 n_seg and d is a mean over 30 frames.
static __global__ __launch_bounds__(WUNET_THREADS) void estoi_segment_kernel(StoiSegArgs A)
{
    constexpr int TBS = (WUNET_STOI_SB + WUNET_STOI_SEG - 1) * WUNET_STOI_BANDS, RS = WUNET_STOI_SB * WUNET_STOI_BANDS;
    __shared__ double tb[2 * TBS];
    __shared__ double rs[4 * RS];        // mean X | r X | mean Y | r Y
    __shared__ double red[WUNET_WAVES];
    const int tid = threadIdx.x;
    const size_t row = blockIdx.y;
    const int nseg = stoi_segments(A.nk[row]), s0 = (int)blockIdx.x * WUNET_STOI_SB;
    if (s0 >= nseg) return;
    const int ns = nseg - s0 < WUNET_STOI_SB ? nseg - s0 : WUNET_STOI_SB;
    estoi_load_bands(A.pw, (size_t)A.M * WUNET_STOI_BP, row, A.Fmax, s0, ns + WUNET_STOI_SEG - 1, tb, TBS);
    __syncthreads();
    for (int i = tid; i < ns * WUNET_STOI_BANDS; i += WUNET_THREADS) {   // (segment i / 15, band i % 15): frame n at + 15 n
        const EstoiRow x = estoi_row(tb + i), y = estoi_row(tb + TBS + i);
        rs[i] = x.m; rs[RS + i] = x.r; rs[2 * RS + i] = y.m; rs[3 * RS + i] = y.r;
    }
    __syncthreads();
    double dsum[1] = {0.0};
    for (int i = tid; i < ns * WUNET_STOI_SEG; i += WUNET_THREADS) {
        const int sl = i / WUNET_STOI_SEG, n = i - sl * WUNET_STOI_SEG;
        const double* st = rs + sl * WUNET_STOI_BANDS;
        const EstoiCol c = estoi_col(tb + (sl + n) * WUNET_STOI_BANDS, tb + TBS + (sl + n) * WUNET_STOI_BANDS, st, st + RS, st + 2 * RS, st + 3 * RS);
        dsum[0] += c.sxy / ((c.nx + WUNET_STOI_EPS) * (c.ny + WUNET_STOI_EPS));
    }
    block_sum<1>(dsum, red);
    if (tid == 0) A.part[row * A.nblk + blockIdx.x] = 0.5 * dsum[0];
}

struct EstoiBwdArgs {
    const float* pw;        // [2][M][BP], as the forward left it
    const int* nk;          // [rows]
    const float* gl;        // grad_loss[0]
    unsigned M, Fmax, nsmax;    // nsmax = Fmax - 29: the most segments a row can have
    double inv_rows;        // 1 / rows
    double* blk;            // [rows][nsmax][30][15]: d d_m / d Y of segment m, written for the segments a row has
    double* gr;             // [M][15]: d loss / d Y divided by Y, written for the frames of the rows that have a segment
};

// d d / d yr[n][j] of one segment through the column normalisation of frame n: with x~ = (xr - cx) / (Nx + EPS), yc = yr - cy, N = |yc|,
// D = N + EPS: x~ / (30 D) - K yc, K = sum_j x~ yc / (30 D^2 N) (its mean over j is 0: the centring passes it unchanged).
// ar = 1 / (30 D (Nx + EPS)); ar = K = 0 where N == 0.
__device__ __forceinline__ double estoi_g2(double x, double y, double mx, double rx, double my, double ry, double cx, double ar, double cy, double k)
{
    return ar * ((x - mx) * rx - cx) - k * ((y - my) * ry - cy);
}

// grid (nsmax / 16 rounded up, rows).  Four stages with a barrier between them, LDS 37 KiB (magnitudes 2 x 45 x 15, row statistics
// 6 x 16 x 15, column statistics 4 x 16 x 30 doubles):
//   1  per (segment, band), one thread each: mean and r of X and Y;
//   2  per (segment, frame): the column means, ar and K of estoi_g2;
//   3  per (segment, band), the threads of stage 1: g = estoi_g2 over the 30 frames -> its mean gm and P = sum g (Y - my) / (D^2 N), with
//      N the row's norm, D = N + EPS; P = 0 and r = 0 where N == 0;
//   4  per (segment, frame, band): d d / d Y = (g - gm) r - P (Y - my), the row normalisation's derivative, into blk.
static __global__ __launch_bounds__(WUNET_THREADS) void estoi_segment_bwd_kernel(EstoiBwdArgs A)
{
    constexpr int TBS = (WUNET_ESTOI_SGB + WUNET_STOI_SEG - 1) * WUNET_STOI_BANDS, RS = WUNET_ESTOI_SGB * WUNET_STOI_BANDS, CS = WUNET_ESTOI_SGB * WUNET_STOI_SEG;
    static_assert(RS <= WUNET_THREADS, "stages 1 and 3 keep a (segment, band) in one thread's registers");
    __shared__ double tb[2 * TBS];
    __shared__ double rs[6 * RS];        // mean X | r X | mean Y | r Y | gm | P
    __shared__ double cs[4 * CS];        // cx | ar | cy | K
    const int tid = threadIdx.x;
    const size_t row = blockIdx.y;
    const int nseg = stoi_segments(A.nk[row]), m0 = (int)blockIdx.x * WUNET_ESTOI_SGB;
    if (m0 >= nseg) return;
    const int ns = nseg - m0 < WUNET_ESTOI_SGB ? nseg - m0 : WUNET_ESTOI_SGB;
    estoi_load_bands(A.pw, (size_t)A.M * WUNET_STOI_BP, row, A.Fmax, m0, ns + WUNET_STOI_SEG - 1, tb, TBS);
    __syncthreads();
    const bool own = tid < ns * WUNET_STOI_BANDS;                        // (segment tid / 15, band tid % 15): frame n at + 15 n
    EstoiRow x{}, y{};
    if (own) {
        x = estoi_row(tb + tid); y = estoi_row(tb + TBS + tid);
        rs[tid] = x.m; rs[RS + tid] = x.r; rs[2 * RS + tid] = y.m; rs[3 * RS + tid] = y.r;
    }
    __syncthreads();
    for (int i = tid; i < ns * WUNET_STOI_SEG; i += WUNET_THREADS) {
        const int sl = i / WUNET_STOI_SEG, n = i - sl * WUNET_STOI_SEG;
        const double* st = rs + sl * WUNET_STOI_BANDS;
        const EstoiCol c = estoi_col(tb + (sl + n) * WUNET_STOI_BANDS, tb + TBS + (sl + n) * WUNET_STOI_BANDS, st, st + RS, st + 2 * RS, st + 3 * RS);
        const double dy = c.ny + WUNET_STOI_EPS, rxn = c.nx > 0.0 ? 1.0 / (c.nx + WUNET_STOI_EPS) : 0.0;
        cs[i] = c.cx;
        cs[CS + i] = c.ny > 0.0 ? rxn / (WUNET_STOI_SEG * dy) : 0.0;
        cs[2 * CS + i] = c.cy;
        cs[3 * CS + i] = c.ny > 0.0 ? c.sxy * rxn / (WUNET_STOI_SEG * dy * dy * c.ny) : 0.0;
    }
    __syncthreads();
    if (own) {
        const double* cf = cs + (tid / WUNET_STOI_BANDS) * WUNET_STOI_SEG;
        double sg = 0.0, sd = 0.0;
#pragma unroll
        for (int n = 0; n < WUNET_STOI_SEG; ++n) {
            const double xv = tb[tid + n * WUNET_STOI_BANDS], yv = tb[TBS + tid + n * WUNET_STOI_BANDS];
            const double g = estoi_g2(xv, yv, x.m, x.r, y.m, y.r, cf[n], cf[CS + n], cf[2 * CS + n], cf[3 * CS + n]);
            sg += g; sd += g * (yv - y.m);
        }
        const double d = y.n + WUNET_STOI_EPS;
        rs[4 * RS + tid] = sg / WUNET_STOI_SEG;
        rs[5 * RS + tid] = y.n > 0.0 ? sd / (d * d * y.n) : 0.0;
    }
    __syncthreads();
    double* out = A.blk + (row * A.nsmax + (size_t)m0) * WUNET_ESTOI_BLK;
    for (int i = tid; i < ns * WUNET_ESTOI_BLK; i += WUNET_THREADS) {
        const int sl = i / WUNET_ESTOI_BLK, r = i - sl * WUNET_ESTOI_BLK, n = r / WUNET_STOI_BANDS, j = r - n * WUNET_STOI_BANDS;
        const int ri = sl * WUNET_STOI_BANDS + j, ci = sl * WUNET_STOI_SEG + n, fi = (sl + n) * WUNET_STOI_BANDS + j;
        const double yv = tb[TBS + fi], my = rs[2 * RS + ri], ry = rs[3 * RS + ri];
        const double g = estoi_g2(tb[fi], yv, rs[ri], rs[RS + ri], my, ry, cs[ci], cs[CS + ci], cs[2 * CS + ci], cs[3 * CS + ci]);
        out[i] = (g - rs[4 * RS + ri]) * ry - rs[5 * RS + ri] * (yv - my);
    }
}

// grid (Fmax * 15 / 256 rounded up, rows).  Frame f, band j: the blocks of the segments max(0, f - 29) .. min(f, n_seg - 1) at [f - m][j], in
// that order; times -grad_loss / (rows n_seg); divided by Y (the forward's sum again), 0 where Y == 0.
static __global__ __launch_bounds__(WUNET_THREADS) void estoi_gather_kernel(EstoiBwdArgs A)
{
    const size_t row = blockIdx.y;
    const int nfr = A.nk[row] - 1, nseg = stoi_segments(A.nk[row]), i = (int)(blockIdx.x * WUNET_THREADS + threadIdx.x);
    if (nseg == 0 || i >= nfr * WUNET_STOI_BANDS) return;
    const int f = i / WUNET_STOI_BANDS, band = i - f * WUNET_STOI_BANDS;
    const size_t fr = row * A.Fmax + (size_t)f;
    const double y = estoi_band(A.pw + ((size_t)A.M + fr) * WUNET_STOI_BP, band);
    const int lo = f - (WUNET_STOI_SEG - 1) > 0 ? f - (WUNET_STOI_SEG - 1) : 0, hi = f < nseg - 1 ? f : nseg - 1;
    double g = 0.0;
    for (int m = lo; m <= hi; ++m) g += A.blk[(row * A.nsmax + (size_t)m) * WUNET_ESTOI_BLK + (f - m) * WUNET_STOI_BANDS + band];
    const double scale = -(double)A.gl[0] * A.inv_rows / (double)nseg;
    A.gr[fr * WUNET_STOI_BANDS + band] = y > 0.0 ? g * scale / y : 0.0;
}
