// Data input, reverberant speech (include/wunet_hip.h: wunet_reverb_windows): every row of the batch is a window of the clean array
// convolved with its own room impulse response - a per-row FIR of up to WUNET_REVERB_MAX_TAPS taps - as an exact fp32 MFMA GEMM.
//
// A 16x16 output tile covers 256 consecutive samples t = t0 + i + 16 j.  With k = k' + 16 j
//   out[t0 + i + 16 j] = sum over -240 <= k' < K of A[i][k'] B[k'][j],   A[i][k'] = x[t0 + i - k'],   B[k'][j] = h[k' + 16 j]
// (h zero outside [0, K)).  A is a Toeplitz read of the source, B does not depend on t0: a wave loads one B fragment per k-step and
// uses it for all WUNET_REVERB_NT tiles it owns, each with its own accumulator - independent chains that cover the MFMA's latency.
// `direct` (the first min(E, K) taps only) is a second accumulator set fed by the same A and by B masked to taps < E, over the k-steps
// that reach such a tap.
//
// reverb_kernel   grid (chunks of WUNET_REVERB_CH samples, batch); one block = one row, one chunk, 4 waves x NT tiles.  The K loop runs in
//                 segments of WUNET_REVERB_KS taps: per segment the block stages the source samples the segment reads (masked loads:
//                 zero in front of the item start and past the window's last sample, so nothing outside the clean array is addressed
//                 and a NaN beside it cannot enter through a zero tap) and the segment's taps into LDS.
// LDS images.  xs is the source REVERSED (xs[q] = x[top - q]) so that a lane's A address grows by 4 words per k-step (one base register,
// immediate offsets); the 16 lanes of a row read consecutive words.  hs is h with one pad word after every 16 (hs[q + q / 16]): the B
// read of lane (k = lane / 16, j = lane % 16) is word k + 17 j (+ the step), 64 different banks.
// The row description is read from device memory (rows[b] = window start, item start, RIR start, RIR taps), no atomics, one fixed
// accumulation order: a captured launch follows its tables and two runs are bit-identical.
#pragma once
#include "wunet_dev.h"
#include "wunet_hip.h"                                                // WUNET_REVERB_MAX_TAPS

#define WUNET_REVERB_NT 2                                            // tiles per wave
#define WUNET_REVERB_CH (WUNET_WAVES * WUNET_REVERB_NT * 256)        // samples per block
#define WUNET_REVERB_KS 2048                                         // k' per staged segment (a multiple of 16)
#define WUNET_REVERB_LEAD 240                                        // the k' < 0 part: 16 (columns - 1)
#define WUNET_REVERB_XS (WUNET_REVERB_CH - 241 + WUNET_REVERB_KS)    // source samples of one segment
#define WUNET_REVERB_HQ (WUNET_REVERB_KS + WUNET_REVERB_LEAD)        // taps of one segment
#define WUNET_REVERB_HS (WUNET_REVERB_HQ + WUNET_REVERB_HQ / 16)
#define WUNET_REVERB_STAGE 8                                         // staging loads a thread keeps in flight

struct ReverbArgs {
    const float* clean_flat;
    const float* rir_flat;
    long long clean_total, rir_total;
    const long long* rows;           // [batch][4]
    int early_taps;                  // E
    int length;                      // L
    float* reverberant;
    float* direct;                   // nullptr or [batch][length]
};

// Row b after clamping: the window x[cs .. cs + L), the first sample `is` of its item (the source is zero in front of it) and the
// response h[0 .. K).  cs into [0, clean_total - L] (mix_row's clamp), is into [0, cs]; the RIR range [hs, hs + K) is cut to its part
// inside [0, rir_total) (bounded first, so that hs + K cannot overflow on a corrupt table), then K to WUNET_REVERB_MAX_TAPS.
struct ReverbRow {
    long long cs, is;
    const float* h;
    int K;
};
__device__ __forceinline__ ReverbRow reverb_row(const ReverbArgs& A, int b)
{
    const long long* r = A.rows + 4 * (size_t)b;
    long long cs = r[0], is = r[1], hs = r[2], K = r[3];
    if (cs < 0) cs = 0;
    if (cs > A.clean_total - A.length) cs = A.clean_total - A.length;
    if (is < 0) is = 0;
    if (is > cs) is = cs;
    if (K < 0) K = 0;
    if (K > A.rir_total) K = A.rir_total;
    if (hs > A.rir_total) hs = A.rir_total;
    if (hs < -A.rir_total) hs = -A.rir_total;
    const long long lo = hs < 0 ? 0 : hs, hi = hs + K < A.rir_total ? hs + K : A.rir_total;
    K = hi > lo ? hi - lo : 0;
    if (K > WUNET_REVERB_MAX_TAPS) K = WUNET_REVERB_MAX_TAPS;
    ReverbRow R;
    R.cs = cs;
    R.is = is;
    R.h = A.rir_flat + lo;
    R.K = (int)K;
    return R;
}

// Groups g0 <= g < g1 of four k-steps (16 k': k' = ka + 16 g + 4 u + lane / 16) of one staged segment for the wave's NT tiles; DIRECT: the
// second accumulator set too.  hq = 17 j + lane / 16 and the 17 words of a group's padded taps give the B address, tap0 = ka + 16 j +
// lane / 16 the tap this lane's B element is at g = 0, u = 0.
template <bool DIRECT>
__device__ __forceinline__ void reverb_groups(const float* xs, const float* hs, const int (&abase)[WUNET_REVERB_NT], int hq, int tap0, int early,
                                              int g0, int g1, wunet_f4 (&acc)[WUNET_REVERB_NT], wunet_f4 (&accd)[WUNET_REVERB_NT])
{
    for (int g = g0; g < g1; ++g) {
        const float* hp = hs + hq + 17 * g;
        float bv[4], av[4][WUNET_REVERB_NT];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            bv[u] = hp[4 * u];
#pragma unroll
            for (int n = 0; n < WUNET_REVERB_NT; ++n) av[u][n] = xs[abase[n] + 16 * g + 4 * u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float bd = DIRECT && tap0 + 16 * g + 4 * u < early ? bv[u] : 0.0f;
#pragma unroll
            for (int n = 0; n < WUNET_REVERB_NT; ++n) {
                acc[n] = wunet_mfma16(av[u][n], bv[u], acc[n]);
                if (DIRECT) accd[n] = wunet_mfma16(av[u][n], bd, accd[n]);
            }
        }
    }
}

static __global__ __launch_bounds__(WUNET_THREADS) void reverb_kernel(ReverbArgs A)
{
    __shared__ float xs[WUNET_REVERB_XS];
    __shared__ float hs[WUNET_REVERB_HS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
    const int b = blockIdx.y, c0 = (int)blockIdx.x * WUNET_REVERB_CH, L = A.length;
    const ReverbRow R = reverb_row(A, b);
    float* rv = A.reverberant + (size_t)b * L;
    float* dr = A.direct ? A.direct + (size_t)b * L : nullptr;
    const int cend = L - c0 < WUNET_REVERB_CH ? L : c0 + WUNET_REVERB_CH;
    if (R.K <= 0) {                                                    // no response: the window's own bits
        const float* x = A.clean_flat + R.cs;
        for (int j = c0 + tid; j < cend; j += WUNET_THREADS) {
            const float v = x[j];
            rv[j] = v;
            if (dr) dr[j] = v;
        }
        return;
    }
    const int early = dr ? (A.early_taps < R.K ? A.early_taps : R.K) : 0;
    const int kend = (R.K + 15) & ~15;                                  // (the k' range in whole groups of 16: fewer than K + 256 in all)
    const long long first = R.cs + c0, xlo = R.is, xhi = R.cs + L - 1;  // the chunk's first sample; the source is zero outside [xlo, xhi]
    const int wt0 = wave * WUNET_REVERB_NT * 256;                       // the wave's first tile inside the chunk
    const bool active = c0 + wt0 < L;
    wunet_f4 acc[WUNET_REVERB_NT], accd[WUNET_REVERB_NT];
    int abase[WUNET_REVERB_NT];
#pragma unroll
    for (int n = 0; n < WUNET_REVERB_NT; ++n) {
        acc[n] = wunet_f4{0.f, 0.f, 0.f, 0.f};
        accd[n] = wunet_f4{0.f, 0.f, 0.f, 0.f};
        abase[n] = (WUNET_REVERB_CH - 256 + 15) - (wt0 + n * 256) - li + lq;
    }
    for (int ka = -WUNET_REVERB_LEAD; ka < kend; ka += WUNET_REVERB_KS) {
        const int span = kend - ka < WUNET_REVERB_KS ? kend - ka : WUNET_REVERB_KS;
        __syncthreads();                                               // the previous segment's reads are done
        // xs[q] = x[top - q]: tile t0, row i, tap k' reads q = (CH - 256 + 15) - t0 - i + (k' - ka), 0 <= q < CH - 241 + span
        const long long top = first + (WUNET_REVERB_CH - 256 + 15) - ka;
        const int nx = WUNET_REVERB_CH - 241 + span, nh = span + WUNET_REVERB_LEAD;
        for (int q0 = tid; q0 < nx; q0 += WUNET_REVERB_STAGE * WUNET_THREADS) {          // (a batch of loads in flight, then their stores)
            float v[WUNET_REVERB_STAGE];
#pragma unroll
            for (int u = 0; u < WUNET_REVERB_STAGE; ++u) {
                const long long p = top - (q0 + u * WUNET_THREADS);
                v[u] = q0 + u * WUNET_THREADS < nx && p >= xlo && p <= xhi ? A.clean_flat[p] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < WUNET_REVERB_STAGE; ++u)
                if (q0 + u * WUNET_THREADS < nx) xs[q0 + u * WUNET_THREADS] = v[u];
        }
        for (int q0 = tid; q0 < nh; q0 += WUNET_REVERB_STAGE * WUNET_THREADS) {
            float v[WUNET_REVERB_STAGE];
#pragma unroll
            for (int u = 0; u < WUNET_REVERB_STAGE; ++u) {
                const int q = q0 + u * WUNET_THREADS, k = ka + q;
                v[u] = q < nh && k >= 0 && k < R.K ? R.h[k] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < WUNET_REVERB_STAGE; ++u) {
                const int q = q0 + u * WUNET_THREADS;
                if (q < nh) hs[q + (q >> 4)] = v[u];
            }
        }
        __syncthreads();
        if (active) {
            const int groups = span >> 4;
            int nd = early > ka ? (early - ka + 15) >> 4 : 0;          // groups that reach a tap below `early`
            if (nd > groups) nd = groups;
            reverb_groups<true>(xs, hs, abase, 17 * li + lq, ka + 16 * li + lq, early, 0, nd, acc, accd);
            reverb_groups<false>(xs, hs, abase, 17 * li + lq, ka + 16 * li + lq, early, nd, groups, acc, accd);
        }
    }
    if (!active) return;
    // lane (lq, li) holds rows 4 lq .. 4 lq + 3 of column li: four consecutive samples
    const bool vec = (L & 3) == 0;
#pragma unroll
    for (int n = 0; n < WUNET_REVERB_NT; ++n) {
        const int j = c0 + wt0 + n * 256 + 16 * li + 4 * lq;
        if (vec) {                                                     // (L % 4 == 0 and j % 4 == 0: j < L means j + 4 <= L)
            if (j < L) {
                wunet_st4(rv + j, acc[n]);
                if (dr) wunet_st4(dr + j, accd[n]);
            }
        } else {
            for (int u = 0; u < 4 && j + u < L; ++u) {
                rv[j + u] = acc[n][u];
                if (dr) dr[j + u] = accd[n][u];
            }
        }
    }
}
