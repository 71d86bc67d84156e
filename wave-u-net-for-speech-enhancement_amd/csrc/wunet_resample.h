// Rational resampling of ragged rows (include/wunet_hip.h: wunet_resample_rows): a polyphase FIR filter whose taps are data.  The rows
// of one call lie anywhere in one flat float32 array and share one rate pair up / down (lowest terms) and one filter h'[0 .. n_taps),
// n_taps = 2 L + 1, the gain `up` folded in.  For the row (in start, T_in, out start, T_out) and m < T_out, with c = m down + L,
// phase = c mod up and i_hi = c / up:
//   out[out start + m] = sum_j h'[phase + up j] x[in start + i_hi - j]   over phase + up j < n_taps, x = 0 outside [0, T_in)
// - scipy.signal.resample_poly(x, up, down, window = h' / up) when T_out = ceil(T_in up / down).  float32 operands, exact products in
// double, the sum in double in increasing j, one rounding to float32 (the rule of stoi_resample_kernel).  Every output is written by
// one thread: no atomics, bit-identical run to run.
//
// What was chosen, and why.
//   * grid (rows, y): a block walks the tiles y, y + gridDim.y, .. of its row and leaves at the row's T_out, read from the table in
//     device memory, so a captured launch follows its table.  y is capped (WUNET_RESAMPLE_BLOCKS blocks in all): the filter is staged
//     once per block, and a 35 KiB table per 2 K outputs would be four times the traffic of the samples themselves.
//   * the whole filter lies in LDS in its memory order, index phase + up j ("tap-major").  A tile of outputs walks through the phases
//     in steps of `down`, so from 160 outputs on every phase is used and a part table would save nothing.  A phase-major copy
//     [phase][j] with an odd row stride puts two lanes on one bank exactly when their phases are congruent mod 32 - and so does this
//     order, where the bank is (phase + up j) mod 32: neither is better, and this one is a straight copy.  With up <= 3 every lane of
//     a wave reads one of at most 3 addresses (a broadcast); with 32 | up (160, 640) the phases of 32 neighbouring outputs are distinct
//     mod 32, conflict free; with up = 441 a half-wave has up to 3 phases on a bank.
//   * a thread owns WUNET_RESAMPLE_OUT = 4 outputs o, o + g, o + 2 g, o + 3 g of the tile with g a multiple of up: they share their
//     phase, so a tap is read and widened once for four products, 1.25 LDS reads per term instead of 2.  ds_read_b32 moves 128 B/clk
//     per CU; at two reads per term the 61 terms of a 48 -> 16 kHz output would cost more LDS cycles than its bytes cost HBM time.
//   * the input under the tile is staged in LDS with zeros outside the row, so the inner loop has no bounds and the terms the
//     definition leaves out are exact zeros added to a double.  Neighbouring lanes read x at a stride of down / up samples: a
//     broadcast when upsampling, conflict free for an odd `down` at up = 1, 2- to 3-way between them.
//   * dword global accesses: a row starts at any sample, the staging loop is coalesced, and each of a thread's 4 stores is one
//     coalesced dword per lane.
//   * measured (profiles/resample_bench.txt): 3.6 to 7.3 times the time of a device copy of the same bytes, 2 to 8 times faster than
//     the same filter from torch's conv1d.  The loop is bound by instruction issue, not by bytes: per trip (4 x 64 terms) the wave
//     issues 5 LDS reads, 5 float -> double conversions, 4 double fma, 5 address updates and the loop's own 2, and a wave64 vector
//     instruction takes 4 cycles on a SIMD.  A variant that kept x in LDS as doubles, padded the filter with zeros to a uniform,
//     unrolled trip count (9 vector instructions per trip instead of 16) was measured 1.2 times SLOWER: it doubles the LDS bytes per
//     term, reads them with the half-rate ds_read2_b64, and its larger tile halves the blocks per CU.  It was taken out again.
// The geometry (g, tile, floats of LDS) has one definition, wunet_lds::resample.
#pragma once
#include "wunet_dev.h"
#include "wunet_lds.h"

#define WUNET_RESAMPLE_OUT 4                     // == wunet_lds::kResampleOut
// (WUNET_RESAMPLE_MAX_TAPS = 2 * 10 * 640 + 1 and WUNET_RESAMPLE_MAX_RATIO = 640, the caps of the entry: include/wunet_hip.h)
#define WUNET_RESAMPLE_LIMIT (1LL << 50)         // samples of an array; m * down stays below 2^60
#define WUNET_RESAMPLE_BLOCKS 2048               // blocks of a launch, about

struct ResampleArgs {
    const float* in;
    long long in_total;
    const long long* rows;       // [n][4]: in start, T_in, out start, T_out
    long long max_out, tiles;    // outputs beyond max_out are not computed; tiles = ceil(max_out / tile)
    int up, down, half;          // half = L
    const float* taps;
    int g, ng, tile, span, ntaps;
    float* out;
    long long out_total;
};

static __global__ __launch_bounds__(WUNET_THREADS) void resample_rows_kernel(ResampleArgs A)
{
    WUNET_DYN_SMEM(smem);
    const long long* r = A.rows + 4 * (size_t)blockIdx.x;
    const long long in_start = r[0], T_in = r[1], out_start = r[2];
    long long T_out = r[3];
    // a row that does not lie inside the arrays is skipped, never addressed (every value is first compared with the array's size,
    // which is below WUNET_RESAMPLE_LIMIT, so no sum overflows)
    if (in_start < 0 || in_start > A.in_total || T_in < 0 || T_in > A.in_total - in_start || out_start < 0 || out_start > A.out_total ||
        T_out < 1 || T_out > A.out_total - out_start)
        return;
    if (T_out > A.max_out) T_out = A.max_out;
    const int tid = threadIdx.x, up = A.up, down = A.down;
    float* hs = smem;
    float* xs = smem + A.ntaps;
    for (int i = tid; i < A.ntaps; i += WUNET_THREADS) hs[i] = A.taps[i];
    const float* x = A.in + in_start;            // (only ever dereferenced at [0, T_in))
    float* y = A.out + out_start;
    const int jobs = A.g * A.ng, per_phase = (A.ntaps - 1) / up;
    for (long long p = blockIdx.y; p < A.tiles; p += gridDim.y) {
        const long long m0 = p * A.tile;
        if (m0 >= T_out) return;                 // (the whole block: T_out is the row's)
        const long long m1 = m0 + A.tile < T_out ? m0 + A.tile : T_out;      // the tile's outputs are [m0, m1)
        const long long span0 = (m0 * down + A.half) / up - per_phase;
        const int need = (int)(((m1 - 1) * down + A.half) / up - span0) + 1;  // <= A.span (wunet_lds::resample_span)
        __syncthreads();                         // the trip before has read xs; the first trip: hs is written
        for (int i = tid; i < need; i += WUNET_THREADS) {
            const long long gi = span0 + i;
            xs[i] = gi >= 0 && gi < T_in ? x[gi] : 0.0f;
        }
        __syncthreads();
        for (int q = tid; q < jobs; q += WUNET_THREADS) {
            const int grp = q / A.g, o0 = q - grp * A.g;
            const long long mq = m0 + o0 + (long long)A.g * WUNET_RESAMPLE_OUT * grp;
            if (mq >= m1) continue;
            const long long c = mq * down + A.half, ihi = c / up;
            const int phase = (int)(c - ihi * up), nj = (A.ntaps - 1 - phase) / up + 1;
            int xi[WUNET_RESAMPLE_OUT];
            double acc[WUNET_RESAMPLE_OUT];
#pragma unroll
            for (int u = 0; u < WUNET_RESAMPLE_OUT; ++u) {
                // output mq + u g: the same phase, i_hi further by u g down / up; one beyond the tile's end repeats output 0 and is not stored
                const long long mu = mq + (long long)u * A.g;
                xi[u] = mu < m1 ? (int)(ihi - span0) + u * (A.g / up) * down : (int)(ihi - span0);
                acc[u] = 0.0;
            }
            const float* hp = hs + phase;
            for (int j = 0; j < nj; ++j) {
                const double h = (double)hp[(size_t)up * j];
#pragma unroll
                for (int u = 0; u < WUNET_RESAMPLE_OUT; ++u) acc[u] += h * (double)xs[xi[u] - j];
            }
#pragma unroll
            for (int u = 0; u < WUNET_RESAMPLE_OUT; ++u)
                if (mq + (long long)u * A.g < m1) y[mq + (long long)u * A.g] = (float)acc[u];
        }
    }
}
