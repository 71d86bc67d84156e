// BSS Eval SDR of one source per row (include/wunet_hip.h: wunet_bss_sdr_forward): mir_eval.separation.bss_eval_sources for a single
// source - the energy of the projection of the estimate e onto the reference s and its delays 0 .. n - 1, over what is left.  With
//   r[k] = sum_t s[t] s[t + k],  b[k] = sum_t s[t] e[t + k]  (k < n, both rows zero outside [0, len)),  E = sum e^2,  G = toeplitz(r)
// solve G c = b; then  P = c'b,  R = E - 2 c'b + c'G c,  SDR = 10 log10(P / R).  R is the residual energy of the c that was found (second
// order in the solver's error), not E - c'b.
//   bss_corr_kernel    grid (segments, rows): a block stages the kBssTile samples of its segment and the n - 1 behind them, s and e,
//                      in LDS as doubles - masked by the row's length, never multiplied by zero - and every thread sums the products of
//                      its two lags over the segment's samples in sample order: one double partial of r, b and E per block
//   bss_solve_kernel   one block per row: the partials in segment order, Levinson's recursion on (r, b) in double with O(n) state in
//                      LDS, the three quadratic forms, one rounding to float32 dB
// A float x float product is exact in double, so r, b and E carry only the rounding of their additions; E is summed by the thread of
// lag 0 in the order of r[0] and b[0], so estimate == reference gives E == r[0] == b[0] bit for bit, c = (1, 0, ..), R = 0 exactly:
// +inf.  Levinson, order m -> m + 1, with a the prediction polynomial (a[0] = 1), eps its error and x the solution so far:
//   k = -(sum_i<m a[i] r[m - i]) / eps;  a'[i] = a[i] + k a[m - i];  eps' = eps (1 - k^2);  x'[i] = x[i] + (b[m] - sum_i<m x[i] r[m - i]) / eps' a'[m - i]
// Thread t keeps a and x of its lags t and t + 256 in registers; the reversed reads go through LDS, a double-buffered so that an order
// costs block_sum's two barriers and one more.  The two inner products of an order are one block_sum<2> (wunet_reduce.h: fixed order).
// 511 dependent orders per row: this launch is latency, not arithmetic ("BSS Eval SDR").
// No atomics, every sum in one fixed order: bit-identical run to run.  A row whose reference or estimate is all zero inside its length,
// or whose length is 0, yields NaN in its own row; nothing is read back.  The geometry has one definition: wunet_lds::bss_corr / bss_solve.
#pragma once
#include "wunet_reduce.h"
#include "wunet_lds.h"

struct BssArgs {
    const float* clean;
    const float* est;
    size_t row_len;
    const long long* lengths;    // nullptr or [rows]: clamped to [0, row_len] here
    int n;                       // filter length, 1 .. wunet_lds::kBssMaxFilter
    unsigned segs;               // segments of a row of row_len samples
    double* part;                // [rows][segs][2 n + 1]: r | b | E
    float* out;                  // [rows], dB
};

__device__ __forceinline__ long long bss_row_length(const BssArgs& A, size_t row)
{
    long long len = (long long)A.row_len;
    if (A.lengths) {
        const long long v = A.lengths[row];
        len = v < 0 ? 0 : (v < len ? v : len);
    }
    return len;
}

// grid = (segs, rows) blocks of WUNET_THREADS threads.  A segment that starts at or behind the row's length writes nothing: the solve
// kernel adds the live segments only.
static __global__ __launch_bounds__(WUNET_THREADS) void bss_corr_kernel(BssArgs A)
{
    constexpr int TILE = wunet_lds::kBssTile;
    const wunet_lds::BssCorr lay = wunet_lds::bss_corr(A.n);
    WUNET_DYN_SMEM(smem);
    double* ss = reinterpret_cast<double*>(smem);
    double* es = ss + lay.es();
    const int tid = threadIdx.x, n = A.n;
    const size_t row = blockIdx.y;
    const long long len = bss_row_length(A, row), t0 = (long long)blockIdx.x * TILE;
    if (t0 >= len) return;
    const long long left = len - t0;                                 // samples of the row from the segment's first on
    const int cnt = left < TILE ? (int)left : TILE;                  // samples of the segment
    const int span = cnt + n - 1;                                    // ... and its halo
    const float* s = A.clean + row * A.row_len + t0;
    const float* e = A.est + row * A.row_len + t0;
    for (int i = tid; i < span; i += WUNET_THREADS) {
        double sv = 0.0, ev = 0.0;
        if (i < left) {
            sv = (double)s[i];
            ev = (double)e[i];
        }
        ss[i] = sv;
        es[i] = ev;
    }
    __syncthreads();
    const int k0 = tid, k1 = tid + WUNET_THREADS;
    const bool own0 = k0 < n, own1 = k1 < n;
    double r0 = 0.0, b0 = 0.0, r1 = 0.0, b1 = 0.0, ee = 0.0;
    for (int t = 0; t < cnt; ++t) {
        const double x = ss[t];
        if (own0) {
            r0 += x * ss[t + k0];
            b0 += x * es[t + k0];
        }
        if (own1) {
            r1 += x * ss[t + k1];
            b1 += x * es[t + k1];
        }
        if (tid == 0) ee += es[t] * es[t];
    }
    double* o = A.part + (row * A.segs + blockIdx.x) * (size_t)(2 * n + 1);
    if (own0) {
        o[k0] = r0;
        o[n + k0] = b0;
    }
    if (own1) {
        o[k1] = r1;
        o[n + k1] = b1;
    }
    if (tid == 0) o[2 * n] = ee;
}

// grid = rows blocks of WUNET_THREADS threads.
static __global__ __launch_bounds__(WUNET_THREADS) void bss_solve_kernel(BssArgs A)
{
    constexpr int TILE = wunet_lds::kBssTile, NP = wunet_lds::kBssMaxFilter;
    constexpr wunet_lds::BssSolve lay = wunet_lds::bss_solve();
    WUNET_DYN_SMEM(smem);
    double* rs = reinterpret_cast<double*>(smem);
    double* bs = rs + lay.bs();
    double* as = rs + lay.as();
    double* red = rs + lay.red();
    const int tid = threadIdx.x, n = A.n;
    const size_t row = blockIdx.x;
    const long long len = bss_row_length(A, row);
    const unsigned live = (unsigned)((len + TILE - 1) / TILE);
    const int i0 = tid, i1 = tid + WUNET_THREADS;
    const bool own0 = i0 < n, own1 = i1 < n;

    // ---- the partials of the live segments, in segment order
    const int stride = 2 * n + 1;
    const double* p = A.part + row * A.segs * (size_t)stride;
    for (int j = tid; j < stride; j += WUNET_THREADS) {
        double acc = 0.0;
        for (unsigned g = 0; g < live; ++g) acc += p[(size_t)g * stride + j];
        if (j < n) rs[j] = acc;
        else if (j < 2 * n) bs[j - n] = acc;
        else rs[lay.energy()] = acc;
    }
    for (int j = tid; j < 2 * NP; j += WUNET_THREADS) as[j] = 0.0;
    __syncthreads();
    const double E = rs[lay.energy()], r00 = rs[0];
    if (!(r00 > 0.0) || !(E > 0.0)) {                // a silent reference or estimate, a row of no samples (or NaN inside): NaN, this row only
        if (tid == 0) A.out[row] = __builtin_nanf("");
        return;
    }

    // ---- Levinson: a and x of this thread's two lags live in registers; as[m & 1] receives the polynomial of order m
    double a0 = tid == 0 ? 1.0 : 0.0, a1 = 0.0;
    double x0 = tid == 0 ? bs[0] / r00 : 0.0, x1 = 0.0;
    double eps = r00;
    if (tid == 0) as[0] = 1.0;
    __syncthreads();
    for (int m = 1; m < n; ++m) {
        const double* ao = as + ((m - 1) & 1) * NP;
        double* an = as + (m & 1) * NP;
        double v[2] = {0.0, 0.0};
        if (i0 < m) {
            const double rv = rs[m - i0];
            v[0] = a0 * rv;
            v[1] = x0 * rv;
        }
        if (i1 < m) {
            const double rv = rs[m - i1];
            v[0] += a1 * rv;
            v[1] += x1 * rv;
        }
        block_sum<2>(v, red);
        const double k = -v[0] / eps;
        // (index m of either buffer is written for the first time in order m: ao[m] is the 0.0 of the start)
        if (i0 <= m) {
            a0 += k * ao[m - i0];
            an[i0] = a0;
        }
        if (own1 && i1 <= m) {
            a1 += k * ao[m - i1];
            an[i1] = a1;
        }
        eps *= 1.0 - k * k;
        __syncthreads();
        const double lam = (bs[m] - v[1]) / eps;
        if (i0 <= m) x0 += lam * an[m - i0];
        if (own1 && i1 <= m) x1 += lam * an[m - i1];
    }

    // ---- P = c'b and c'G c (n^2 terms: thread i forms c_i sum_j c_j r[|i - j|], j ascending), R, the score
    __syncthreads();
    double* cs = as;
    if (own0) cs[i0] = x0;
    if (own1) cs[i1] = x1;
    __syncthreads();
    double v[2] = {0.0, 0.0};
    if (own0) {
        double g = 0.0;
        for (int j = 0; j < n; ++j) g += cs[j] * rs[j < i0 ? i0 - j : j - i0];
        v[0] = x0 * bs[i0];
        v[1] = x0 * g;
    }
    if (own1) {
        double g = 0.0;
        for (int j = 0; j < n; ++j) g += cs[j] * rs[j < i1 ? i1 - j : j - i1];
        v[0] += x1 * bs[i1];
        v[1] += x1 * g;
    }
    block_sum<2>(v, red);
    if (tid == 0) {
        double R = (E - 2.0 * v[0]) + v[1];
        R = R < 0.0 ? 0.0 : R;                       // (the rounding of a full cancellation may land below 0)
        A.out[row] = (float)(10.0 * log10(v[0] / R));
    }
}
