// Row-structured losses: scale-invariant SDR and SNR per utterance (include/wunet_hip.h: wunet_loss_rows_*).  The three element-wise
// means of wunet_loss_mean.h treat the batch as one flat array; these reduce every row (the last dimension, T samples) on its own.
//   loss_rows_partial_kernel   one pass over the pair: a block reduces one piece of one row to five raw sums, in double
//   loss_rows_final_kernel     the pieces of each row in piece order -> centred moments -> v [dB] and the gradient coefficients; the loss
//   loss_rows_bwd_kernel       g[i] = -grad_loss / R * (A_r e[i] + C_r s[i] + D_r), applied in its centred form, streaming
// Why double: the noise energy  r - 2 alpha p + alpha^2 q  (and the centring  sum x^2 - (sum x)^2 / T) cancels - at 57 dB all but 2e-6
// of it, which fp32 sums do not survive ("Row losses").  A float x float product is exact in double, so the raw sums carry
// only the rounding of their additions.  No atomics anywhere: every sum has one fixed order, results are bit-identical run to run.
#pragma once
#include "wunet_reduce.h"
#include "wunet_row_piece.h"

#define WUNET_ROWS_SUMS 5            // per piece: sum s, sum x, sum s^2, sum x^2, sum x s   (x = e for si_sdr, e - s for snr)
#define WUNET_ROWS_KIND_SNR 4        // == WUNET_LOSS_SNR
#define WUNET_ROWS_COEFS 6           // == WUNET_LOSS_ROW_COEFS: A, C, D, v, mean of x, mean of s (0 without zero_mean)

// one sample pair into the five sums.  (double)s * (double)s is exact (24 x 24 bits), so contracting it into an fma changes nothing.
__device__ __forceinline__ void loss_rows_acc(bool snr, float sf, float ef, double (&a)[WUNET_ROWS_SUMS])
{
    const double s = (double)sf, e = (double)ef;
    const double x = snr ? e - s : e;            // snr: the noise energy is accumulated from the differences themselves
    a[0] += s;
    a[1] += x;
    a[2] += s * s;
    a[3] += x * x;
    a[4] += x * s;
}

// How many leading samples of a piece go the scalar way so that the rest starts on a 16-byte boundary; -1: the pointers disagree
// modulo 16 (only 4-byte alignment in common) and the whole piece is scalar.
__device__ __forceinline__ int loss_rows_head(const void* p0, const void* p1, const void* p2)
{
    const unsigned m0 = (unsigned)((size_t)p0 & 15), m1 = (unsigned)((size_t)p1 & 15), m2 = p2 ? (unsigned)((size_t)p2 & 15) : m0;
    if (m0 != m1 || m0 != m2 || (m0 & 3)) return -1;
    return (int)((16 - m0) >> 2) & 3;
}

// One piece of one row: n samples at s and e (and g, the output of the backward, or nullptr).  Pointers that agree modulo 16 take the
// 16-byte way: op.four(i, s[i .. i + 3], e[i .. i + 3]) on every aligned group of four, the eight loads of four trips issued before the
// first is used (loss_partial_kernel's comment: one trip at a time is one dependent memory round trip per trip), op.one(i, s[i], e[i])
// on the at most three samples before and after them.  Otherwise - a base that is only 4-byte aligned, or rows of odd length whose
// pointers fall apart - op.one on every sample, four trips in flight.  A thread meets its samples in one fixed order: the head
// element, the tail element, then its trips in trip order.
template <class Op>
__device__ __forceinline__ void loss_rows_walk(const float* s, const float* e, const void* g, size_t n, Op& op)
{
    const int tid = threadIdx.x;
    const int head = loss_rows_head(s, e, g);
    if (head < 0) {
        size_t i = tid;
        for (; i + 3 * WUNET_THREADS < n; i += 4 * WUNET_THREADS) {
            float sv[4], ev[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { sv[u] = s[i + u * WUNET_THREADS]; ev[u] = e[i + u * WUNET_THREADS]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) op.one(i + u * WUNET_THREADS, sv[u], ev[u]);
        }
        for (; i < n; i += WUNET_THREADS) op.one(i, s[i], e[i]);
        return;
    }
    const size_t h = (size_t)head < n ? (size_t)head : n;
    const size_t nvec = (n - h) >> 2, tail = h + (nvec << 2);
    if ((size_t)tid < h) op.one(tid, s[tid], e[tid]);
    if (tail + tid < n) op.one(tail + tid, s[tail + tid], e[tail + tid]);
    size_t v = tid;
    for (; v + 3 * WUNET_THREADS < nvec; v += 4 * WUNET_THREADS) {
        wunet_f4 sv[4], ev[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { sv[u] = wunet_ld4(s + h + ((v + u * WUNET_THREADS) << 2)); ev[u] = wunet_ld4(e + h + ((v + u * WUNET_THREADS) << 2)); }
#pragma unroll
        for (int u = 0; u < 4; ++u) op.four(h + ((v + u * WUNET_THREADS) << 2), sv[u], ev[u]);
    }
    for (; v < nvec; v += WUNET_THREADS) {
        const wunet_f4 sv = wunet_ld4(s + h + (v << 2)), ev = wunet_ld4(e + h + (v << 2));
        op.four(h + (v << 2), sv, ev);
    }
}

// the forward's op: every sample pair into the five raw sums
struct LossRowsSumOp {
    bool snr;
    double a[WUNET_ROWS_SUMS];
    __device__ __forceinline__ void one(size_t, float sf, float ef) { loss_rows_acc(snr, sf, ef, a); }
    __device__ __forceinline__ void four(size_t, const wunet_f4& sv, const wunet_f4& ev)
    {
#pragma unroll
        for (int j = 0; j < 4; ++j) loss_rows_acc(snr, sv[j], ev[j], a);
    }
};

// grid = rows * ppr blocks (block = row * ppr + piece); piece p of a row is samples [p * plen, min(T, (p + 1) * plen)), plen a multiple
// of 4 chosen by the host from (rows, T): no block is empty.  part[block][WUNET_ROWS_SUMS].
static __global__ __launch_bounds__(WUNET_THREADS) void loss_rows_partial_kernel(int kind, const float* clean, const float* enh, size_t T,
                                                                           unsigned ppr, size_t plen, double* part)
{
    __shared__ double red[WUNET_ROWS_SUMS * WUNET_WAVES];
    const RowPiece P = row_piece(blockIdx.x / ppr, blockIdx.x % ppr, plen, T);
    LossRowsSumOp op{kind == WUNET_ROWS_KIND_SNR, {0.0, 0.0, 0.0, 0.0, 0.0}};
    loss_rows_walk(clean + P.row * T + P.beg, enh + P.row * T + P.beg, nullptr, P.end - P.beg, op);
    block_sum<WUNET_ROWS_SUMS>(op.a, red);
    if (threadIdx.x == 0) {
        double* o = part + (size_t)blockIdx.x * WUNET_ROWS_SUMS;
#pragma unroll
        for (int k = 0; k < WUNET_ROWS_SUMS; ++k) o[k] = op.a[k];
    }
}

struct LossRowsFinalArgs {
    const double* part;     // [rows][ppr][WUNET_ROWS_SUMS]
    size_t rows, T;
    unsigned ppr;
    int group;              // lanes per row: a power of two 1 .. 64, >= min(ppr, 64)
    int kind, zero_mean;
    double eps;
    float* loss;            // -mean over rows of v
    float* per_row;         // nullptr or [rows]: v in dB
    double* coefs;          // nullptr or [rows][WUNET_ROWS_COEFS]: A, C, D, v, mx, ms   (dv/de[i] = A e[i] + C s[i] + D)
};

// ONE block.  A row is owned by `group` neighbouring lanes of a wave: lane j adds pieces j, j + group, ... in that order, a butterfly
// over the group adds the lanes' sums (fixed order), the group's first lane forms the centred moments, v and the coefficients.  The
// block walks the rows 256 / group at a time - any row count - and every thread keeps the sum of the v it wrote; block_sum ends it.
static __global__ __launch_bounds__(WUNET_THREADS) void loss_rows_final_kernel(LossRowsFinalArgs A)
{
    __shared__ double red[WUNET_WAVES];
    const int tid = threadIdx.x, G = A.group;
    const int lane_in = tid & (G - 1);
    const size_t per_pass = (size_t)(WUNET_THREADS / G);
    const bool snr = A.kind == WUNET_ROWS_KIND_SNR;
    const double Td = (double)A.T;
    double vsum[1] = {0.0};
    for (size_t base = 0; base < A.rows; base += per_pass) {          // (uniform trip count: the shuffles below need every lane)
        const size_t row = base + (size_t)(tid / G);
        const bool live = row < A.rows;
        double a[WUNET_ROWS_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (live) {
            const double* p = A.part + row * A.ppr * WUNET_ROWS_SUMS;
            for (unsigned k = lane_in; k < A.ppr; k += G) {
#pragma unroll
                for (int q = 0; q < WUNET_ROWS_SUMS; ++q) a[q] += p[(size_t)k * WUNET_ROWS_SUMS + q];
            }
        }
        for (int m = G >> 1; m > 0; m >>= 1) {
#pragma unroll
            for (int q = 0; q < WUNET_ROWS_SUMS; ++q) a[q] += wunet_shfl_xor_d(a[q], m);
        }
        if (!live || lane_in != 0) continue;
        // centred moments (zero_mean) of s and x from the raw sums
        const double ms = A.zero_mean ? a[0] / Td : 0.0, mx = A.zero_mean ? a[1] / Td : 0.0;
        double q = a[2] - ms * a[0], r = a[3] - mx * a[1];
        const double p = a[4] - ms * a[1];
        q = q < 0.0 ? 0.0 : q;
        r = r < 0.0 ? 0.0 : r;
        const double k10 = 4.342944819032518;                         // 10 / ln 10
        double Et, En, ca, cc, cd;
        if (snr) {
            // x = e - s: Et = q, En = r;  dv/de = -(2 k10 / (En + eps)) (x - mx)
            Et = q; En = r;
            ca = -2.0 * k10 / (En + A.eps);
            cc = -ca;
            cd = -ca * mx;
        } else {
            const double al = p / (q + A.eps), be = q / (q + A.eps);
            Et = al * al * q;
            En = r - 2.0 * al * p + al * al * q;
            En = En < 0.0 ? 0.0 : En;                                  // (|| e - alpha s ||^2: the rounding of a full cancellation may land below 0)
            // dv/d(e - me) = A (e - me) + C (s - ms); both centred, so the centring of the gradient changes nothing
            ca = -2.0 * k10 / (En + A.eps);
            cc = 2.0 * k10 * al * (be / (Et + A.eps) + (2.0 - be) / (En + A.eps));
            cd = -ca * mx - cc * ms;
        }
        const double v = 10.0 * log10((Et + A.eps) / (En + A.eps));
        vsum[0] += v;
        if (A.per_row) A.per_row[row] = (float)v;
        if (A.coefs) {
            double* o = A.coefs + row * WUNET_ROWS_COEFS;
            o[0] = ca; o[1] = cc; o[2] = cd; o[3] = v; o[4] = mx; o[5] = ms;
        }
    }
    block_sum<1>(vsum, red);
    if (tid == 0) *A.loss = (float)(-vsum[0] / (double)A.rows);
}

// grad_enh[row][i] = gscale[0] * (-1 / rows) * (A e + C s + D): the coefficients applied in double, one rounding to float (A e and C s
// cancel as e -> alpha s; applied in fp32 they leave 1e-4 of the gradient at 57 dB).  D = -A mx - C ms is the centring, and it is applied
// as such - si_sdr: A (e - mx) + C (s - ms), snr: A ((e - s) - mx) - not as a third term: next to A e (2 k / eps = 9e8 times e on a row
// without noise energy) the rounding of a separately formed D is 1e-16 of THAT, 1e-8 where the gradient is exactly 0 (a row of one
// sample; every sample equal to the row's mean).  The differences are exact or rounded relative to themselves.
// The backward's op, then its kernel: the same (row, piece) grid as the partial kernel.
struct LossRowsGradOp {
    bool snr;
    double ca, cc, mx, ms;
    float* g;
    // snr: x = e - s as the forward formed it, C = -A folded into x;  si_sdr: x = e
    // (one fma asked for by name: the scalar and the 16-byte paths then round alike whatever the compiler contracts elsewhere)
    __device__ __forceinline__ float grad(float sf, float ef) const
    {
        return (float)fma(ca, ((double)ef - (snr ? (double)sf : 0.0)) - mx, cc * ((double)sf - ms));
    }
    __device__ __forceinline__ void one(size_t i, float sf, float ef) { g[i] = grad(sf, ef); }
    __device__ __forceinline__ void four(size_t i, const wunet_f4& sv, const wunet_f4& ev)
    {
        wunet_f4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = grad(sv[j], ev[j]);
        wunet_st4(g + i, o);
    }
};

static __global__ __launch_bounds__(WUNET_THREADS) void loss_rows_bwd_kernel(int kind, const float* clean, const float* enh, const double* coefs,
                                                                       const float* gscale, size_t rows, size_t T, unsigned ppr,
                                                                       size_t plen, float* genh)
{
    const bool snr = kind == WUNET_ROWS_KIND_SNR;
    const RowPiece P = row_piece(blockIdx.x / ppr, blockIdx.x % ppr, plen, T);
    const double sc = -(double)gscale[0] / (double)rows;
    const double* co = coefs + P.row * WUNET_ROWS_COEFS;
    LossRowsGradOp op{snr, sc * co[0], snr ? 0.0 : sc * co[1], co[4], co[5], genh + P.row * T + P.beg};
    loss_rows_walk(clean + P.row * T + P.beg, enh + P.row * T + P.beg, op.g, P.end - P.beg, op);
}
