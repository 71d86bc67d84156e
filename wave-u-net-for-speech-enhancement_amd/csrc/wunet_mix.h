// Data input.  Aligned crops (include/wunet_hip.h: wunet_crop_windows):
//   crop_windows_kernel  the (mixture, clean) windows of a batch out of two flat arrays, one launch
// On-the-fly mixing (wunet_mix_windows): a batch of clean windows and a batch of noise windows gathered
// from two flat float32 arrays resident in HBM, mixed at a per-row SNR and level that the host drew.
//   mix_partial_kernel   one pass over both windows: a block reduces one piece of one row to sum c^2, sum n^2 (double), max|c|, max|n|
//   mix_apply_kernel     every block folds its row's partials in piece order -> g, a (double, rounded once to float32), then
//                        mixture = a (c + g n), clean_out = a c over its piece
//   apply_level_kernel   dst = a src for the a of a gains table (wunet_apply_level): the multiply of clean_out, for a target that is not
//                        the window the mix read
// The row description is read from device memory (rows[b] = clean start, noise item start, noise item length, noise phase; params[b] =
// snr_db, level), so a captured pair of launches follows the tables it was captured on.  The sums use block_sum's fixed order and the
// partials are folded in piece order by every block on its own: no atomics, bit-identical run to run.  Window starts are any sample,
// so the loads are dwords (crop_windows_kernel's reasoning); a thread owns 4 consecutive samples and stores one float4 per output when
// the row length allows it.
#pragma once
#include "wunet_reduce.h"
#include "wunet_row_piece.h"

// ---------------------------------------------------------------------------- data input: aligned window crops (f4)
// out[b][j] = flat[starts[b] + j] for the mixture and the clean array alike (the reference's sample_fixed_length_data_aligned,
// util/utils.py:101-113, for a whole batch).  A window start is any sample, so the loads are dwords (64 consecutive per wave
// instruction: coalesced, never 16-byte aligned in general); a thread gathers 4 consecutive samples and stores them as one
// aligned float4 per array when the row length allows it.  HBM-bound: 16 B read + 16 B written per thread.
static __global__ __launch_bounds__(WUNET_THREADS) void crop_windows_kernel(const float* mix_flat, const float* clean_flat, const long long* starts,
                                                                            long long total, int length, float* mix, float* clean)
{
    const int b = blockIdx.y;
    long long s0 = starts[b];
    if (s0 < 0) s0 = 0;                                   // (a corrupt start must not read outside the shard)
    if (s0 > total - length) s0 = total - length;
    const int j0 = (blockIdx.x * WUNET_THREADS + threadIdx.x) * 4;
    if (j0 >= length) return;
    const float* ms = mix_flat + s0 + j0;
    const float* cs = clean_flat + s0 + j0;
    float* md = mix + (size_t)b * length + j0;
    float* cd = clean + (size_t)b * length + j0;
    if (j0 + 4 <= length && (length & 3) == 0) {
        const wunet_f4 m = {ms[0], ms[1], ms[2], ms[3]};
        const wunet_f4 c = {cs[0], cs[1], cs[2], cs[3]};
        wunet_st4(md, m);
        wunet_st4(cd, c);
    } else {
        for (int k = 0; k < 4 && j0 + k < length; ++k) { md[k] = ms[k]; cd[k] = cs[k]; }
    }
}

// ---------------------------------------------------------------------------- mixtures made on the device
#define WUNET_MIX_PART 4             // per piece: sum c^2, sum n^2, max|c|, max|n| (all kept as double)
#define WUNET_MIX_SILENT 1e-12       // mean square below which a window counts as silent (RMS 1e-6)

struct MixArgs {
    const float* clean_flat;
    const float* noise_flat;
    long long clean_total, noise_total;
    const long long* rows;           // [batch][4]
    const float* params;             // [batch][2]
    float peak_limit;
    int length;                      // L
    unsigned ppr;                    // pieces per row
    int plen;                        // samples per piece, a multiple of 4
    double* part;                    // [batch][ppr][WUNET_MIX_PART]
    float* mixture;
    float* clean_out;
    float* gains;                    // nullptr or [batch][2]
};

// The two windows of row b after clamping: c[0 .. L) and the noise item n[0 .. nl) read circularly from phase ph.  nl == 0: no noise.
// Clean start: into [0, clean_total - L] (crop_windows_kernel's clamp).  Noise item: [ns, ns + nl) cut to its part inside
// [0, noise_total); the phase is reduced modulo the length that is left.  Nothing outside either array is ever addressed.
struct MixRow {
    const float* c;
    const float* n;
    long long nl, ph;
};
__device__ __forceinline__ MixRow mix_row(const MixArgs& A, int b)
{
    const long long* r = A.rows + 4 * (size_t)b;
    long long cs = r[0], ns = r[1], nl = r[2], ph = r[3];
    if (cs < 0) cs = 0;
    if (cs > A.clean_total - A.length) cs = A.clean_total - A.length;
    // (bounded first, so that ns + nl cannot overflow on a corrupt table)
    if (nl < 0) nl = 0;
    if (nl > A.noise_total) nl = A.noise_total;
    if (ns > A.noise_total) ns = A.noise_total;
    if (ns < -A.noise_total) ns = -A.noise_total;
    const long long lo = ns < 0 ? 0 : ns, hi = ns + nl < A.noise_total ? ns + nl : A.noise_total;
    nl = hi > lo ? hi - lo : 0;
    if (nl > 0) {
        ph %= nl;
        if (ph < 0) ph += nl;
    } else {
        ph = 0;
    }
    MixRow R;
    R.c = A.clean_flat + cs;
    R.n = A.noise_flat + lo;
    R.nl = nl;
    R.ph = ph;
    return R;
}

// grid = batch * ppr blocks (block = row * ppr + piece); piece p of a row is samples [p * plen, min(L, (p + 1) * plen)).  A thread takes
// samples j0 .. j0 + 3, j0 = beg + 4 (tid + 256 trip); its position inside the noise item moves by (1024 mod nl) per trip.
static __global__ __launch_bounds__(WUNET_THREADS) void mix_partial_kernel(MixArgs A)
{
    __shared__ double red[2 * WUNET_WAVES];
    const RowPiece P = row_piece(blockIdx.x / A.ppr, blockIdx.x % A.ppr, (size_t)A.plen, (size_t)A.length);
    const int b = (int)P.row, beg = (int)P.beg, end = (int)P.end, tid = threadIdx.x;
    const MixRow R = mix_row(A, b);
    const bool noisy = R.nl > 0;
    long long k = noisy ? (R.ph + beg + 4 * tid) % R.nl : 0;
    const long long step = noisy ? (long long)(4 * WUNET_THREADS) % R.nl : 0;
    double pc = 0.0, pn = 0.0;
    float mc = 0.0f, mn = 0.0f;
    for (int j0 = beg + 4 * tid; j0 < end; j0 += 4 * WUNET_THREADS) {
        long long kk = k;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (j0 + u < end) {
                const float cv = R.c[j0 + u];
                pc += (double)cv * (double)cv;
                mc = fmaxf(mc, fabsf(cv));
                if (noisy) {
                    const float nv = R.n[kk];
                    pn += (double)nv * (double)nv;
                    mn = fmaxf(mn, fabsf(nv));
                    if (++kk == R.nl) kk = 0;
                }
            }
        }
        k += step;
        if (k >= R.nl) k -= R.nl;
    }
    block_sum2(pc, pn, red);
    block_max2(mc, mn, red);
    if (tid == 0) {
        double* o = A.part + (size_t)blockIdx.x * WUNET_MIX_PART;
        o[0] = pc; o[1] = pn; o[2] = (double)mc; o[3] = (double)mn;
    }
}

// grid = (ppr, batch).  Every thread folds the row's partials itself (the same addresses in every lane: broadcast loads, no LDS, no
// barrier), in piece order, and derives g and a in double; the peak guard bounds max|a (c + g n)| by a (max|c| + g max|n|), which needs
// no pass over the mixed row.  g and a are rounded to float32 once; a row without noise (g == 0) writes a c to both outputs.
static __global__ __launch_bounds__(WUNET_THREADS) void mix_apply_kernel(MixArgs A)
{
    const RowPiece P = row_piece(blockIdx.y, blockIdx.x, (size_t)A.plen, (size_t)A.length);
    const int b = (int)P.row, piece = (int)P.piece, beg = (int)P.beg, end = (int)P.end, tid = threadIdx.x;
    const MixRow R = mix_row(A, b);
    double Pc = 0.0, Pn = 0.0, Mc = 0.0, Mn = 0.0;
    const double* p = A.part + (size_t)b * A.ppr * WUNET_MIX_PART;
    for (unsigned q = 0; q < A.ppr; ++q) {
        Pc += p[q * WUNET_MIX_PART];
        Pn += p[q * WUNET_MIX_PART + 1];
        Mc = fmax(Mc, p[q * WUNET_MIX_PART + 2]);
        Mn = fmax(Mn, p[q * WUNET_MIX_PART + 3]);
    }
    const double floor_ = (double)A.length * WUNET_MIX_SILENT;
    double g = 0.0;
    // (written so that a NaN sum fails the test and leaves g = 0)
    if (R.nl > 0 && Pc >= floor_ && Pn >= floor_) g = sqrt(Pc / (Pn * pow(10.0, (double)A.params[2 * b] / 10.0)));
    double a = (double)A.params[2 * b + 1];
    if (A.peak_limit > 0.0f) {
        const double bound = a * (Mc + g * Mn);
        if (bound > (double)A.peak_limit) a = a * (double)A.peak_limit / bound;
    }
    const float gf = (float)g, af = (float)a;
    if (A.gains && piece == 0 && tid == 0) {
        A.gains[2 * b] = gf;
        A.gains[2 * b + 1] = af;
    }
    const bool noisy = gf != 0.0f;
    const bool vec = (A.length & 3) == 0;
    long long k = noisy ? (R.ph + beg + 4 * tid) % R.nl : 0;
    const long long step = noisy ? (long long)(4 * WUNET_THREADS) % R.nl : 0;
    float* md = A.mixture + (size_t)b * A.length;
    float* cd = A.clean_out + (size_t)b * A.length;
    for (int j0 = beg + 4 * tid; j0 < end; j0 += 4 * WUNET_THREADS) {
        long long kk = k;
        wunet_f4 m, c;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            m[u] = 0.0f; c[u] = 0.0f;
            if (j0 + u < end) {
                const float cv = R.c[j0 + u];
                c[u] = af * cv;
                if (noisy) {
                    // (one fma asked for by name: the GPU build and the emulator build round alike)
                    m[u] = af * fmaf(gf, R.n[kk], cv);
                    if (++kk == R.nl) kk = 0;
                } else {
                    m[u] = c[u];
                }
            }
        }
        if (vec) {                                      // (L % 4 == 0: every piece ends on a multiple of 4, j0 + 4 <= end)
            wunet_st4(md + j0, m);
            wunet_st4(cd + j0, c);
        } else {
            for (int u = 0; u < 4 && j0 + u < end; ++u) { md[j0 + u] = m[u]; cd[j0 + u] = c[u]; }
        }
        k += step;
        if (k >= R.nl) k -= R.nl;
    }
}

// grid = (pieces of 4 * WUNET_THREADS samples, batch).  dst[b][j] = gains[b][1] * src[b][j]: mix_apply_kernel's one float32 multiply, so a
// row scaled here equals that kernel's a c bit for bit.  A thread reads its four samples before it writes them: dst == src is allowed.
static __global__ __launch_bounds__(WUNET_THREADS) void apply_level_kernel(const float* src, const float* gains, int length, float* dst)
{
    const int b = blockIdx.y, j0 = 4 * ((int)blockIdx.x * WUNET_THREADS + (int)threadIdx.x);
    if (j0 >= length) return;
    const float af = gains[2 * b + 1];
    const float* s = src + (size_t)b * length;
    float* d = dst + (size_t)b * length;
    if ((length & 3) == 0) {
        wunet_f4 v = wunet_ld4(s + j0);
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = af * v[u];
        wunet_st4(d + j0, v);
    } else {
        for (int u = 0; u < 4 && j0 + u < length; ++u) d[j0 + u] = af * s[j0 + u];
    }
}
