// Chunked enhancement with overlap (include/wunet_hip.h: wunet_chunk_gather, wunet_chunk_overlap_add): the recordings of one call lie
// back to back in one flat float32 array; the model sees rows of L samples that overlap by 2 m + f, and the outputs are put back
// together with a margin of m samples dropped at every chunk edge and a cross-fade of f samples between neighbours.
//   chunk_gather_kernel        chunks[i][j] = flat[start + s + j] inside the recording (rows[i] = start, T, s), 0 outside it
//   chunk_overlap_add_kernel   out[start + t] for t < T of every recording (recs[r] = start, T, first chunk row, chunk count): a copy of
//                              one chunk's sample outside the cross-fades, ramp[j] y_k + (1 - ramp[j]) y_(k-1) inside them
// Everything ragged is read from device memory, so a captured launch follows its tables.  Every output sample is written by exactly one
// thread from at most two inputs: no atomics, bit-identical run to run.  Both kernels move 4 bytes in and 4 bytes out per sample and are
// bound by that traffic: a thread owns 4 consecutive samples and moves them as one 16-byte load and one 16-byte store when every
// address involved is 16-byte aligned (a recording starts at any sample of the flat array, so that is tested, not assumed) and as
// dwords otherwise.  Loads outside a recording or outside the flat array are masked, never made and multiplied by zero.
#pragma once
#include "wunet_dev.h"

#define WUNET_CHUNK_PIECE (4 * WUNET_THREADS)    // samples per block and trip
#define WUNET_CHUNK_MAX_Y 65535u                 // blocks along a row; longer rows take further trips
#define WUNET_CHUNK_LIMIT (1LL << 56)            // table entries beyond it are corrupt: the row is treated as empty

__device__ __forceinline__ bool chunk_aligned16(const void* p) { return ((size_t)p & 15) == 0; }

// grid = (n, min(pieces of L, WUNET_CHUNK_MAX_Y)).  Row i reads flat[start + s + j] for the j inside [lo, hi): the part of the chunk
// that lies inside the recording [0, T) and inside the flat array [0, total).
static __global__ __launch_bounds__(WUNET_THREADS) void chunk_gather_kernel(const float* flat, long long total, const long long* rows, int length,
                                                                            float* chunks)
{
    const size_t i = blockIdx.x;
    long long start = rows[3 * i], T = rows[3 * i + 1], s = rows[3 * i + 2];
    if (start < -WUNET_CHUNK_LIMIT || start > WUNET_CHUNK_LIMIT || s < -WUNET_CHUNK_LIMIT || s > WUNET_CHUNK_LIMIT || T < 0 || T > WUNET_CHUNK_LIMIT) T = 0;
    // 0 <= s + j < T and 0 <= start + s + j < total
    long long lo = -s > 0 ? -s : 0, hi = T - s < length ? T - s : length;
    if (-(start + s) > lo) lo = -(start + s);
    if (total - (start + s) < hi) hi = total - (start + s);
    const float* src = flat + (start + s);               // (only ever dereferenced at [lo, hi))
    float* dst = chunks + i * (size_t)length;
    const bool vec_st = (length & 3) == 0 && chunk_aligned16(dst), vec_ld = chunk_aligned16(src);
    for (int j0 = 4 * ((int)blockIdx.y * WUNET_THREADS + (int)threadIdx.x); j0 < length; j0 += 4 * (int)gridDim.y * WUNET_THREADS) {
        wunet_f4 v;
        if (vec_ld && j0 >= lo && j0 + 4 <= hi) {
            v = wunet_ld4(src + j0);
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = 0.0f;
                if (j0 + u >= lo && j0 + u < hi) v[u] = src[j0 + u];
            }
        }
        if (vec_st) {                                    // (L % 4 == 0: j0 + 4 <= L)
            wunet_st4(dst + j0, v);
        } else {
            for (int u = 0; u < 4 && j0 + u < length; ++u) dst[j0 + u] = v[u];
        }
    }
}

struct ChunkOlaArgs {
    const float* chunks;             // [n][length]
    long long n;
    int length, margin, fade, hop;   // L, m, f, H = L - 2 m - f
    const float* ramp;               // [fade], nullptr when fade == 0
    const long long* recs;           // [n_recs][4]
    long long pieces;                // pieces of WUNET_CHUNK_PIECE samples in the longest recording
    float* out_flat;
    long long total;
};

// One output sample: chunk k of the recording (row `first + k` of chunks) at offset j of its trusted span.  false: a row outside [0, n)
// or an offset outside the chunk (a table that does not match the geometry) - the sample is skipped.
__device__ __forceinline__ bool chunk_ola_one(const ChunkOlaArgs& A, long long first, long long k, long long j, float& o)
{
    const long long row = first + k;
    if (row < 0 || row >= A.n || A.margin + j >= A.length) return false;
    const float a = A.chunks[(size_t)row * A.length + A.margin + j];
    if (k >= 1 && j < A.fade) {
        if (row < 1) return false;
        const float b = A.chunks[(size_t)(row - 1) * A.length + A.margin + A.hop + j];
        const float w = A.ramp[j], q = 1.0f - w;
        // (one fma asked for by name: the GPU build and the emulator build round alike)
        o = fmaf(w, a, q * b);
    } else {
        o = a;
    }
    return true;
}

// grid = (n_recs, min(pieces, WUNET_CHUNK_MAX_Y)).  A thread owns samples t0 .. t0 + 3 of its recording.  When the four lie in one
// chunk and on one side of a cross-fade's end they are one 16-byte access per array involved, if those addresses are aligned.
static __global__ __launch_bounds__(WUNET_THREADS) void chunk_overlap_add_kernel(ChunkOlaArgs A)
{
    const long long* r = A.recs + 4 * (size_t)blockIdx.x;
    const long long start = r[0], T = r[1] > WUNET_CHUNK_LIMIT ? 0 : r[1], first = r[2], count = r[3];
    if (count < 1 || count > WUNET_CHUNK_LIMIT || start < -WUNET_CHUNK_LIMIT || start > WUNET_CHUNK_LIMIT || first < -WUNET_CHUNK_LIMIT ||
        first > WUNET_CHUNK_LIMIT)
        return;
    const long long H = A.hop;
    for (long long p = blockIdx.y; p < A.pieces; p += gridDim.y) {
        const long long t0 = p * WUNET_CHUNK_PIECE + 4 * (long long)threadIdx.x;
        if (t0 >= T) return;
        long long k0 = t0 / H;
        if (k0 > count - 1) k0 = count - 1;
        const long long j0 = t0 - k0 * H, g0 = start + t0;
        float* dst = A.out_flat + g0;
        const bool whole = t0 + 4 <= T && g0 >= 0 && g0 + 4 <= A.total && (j0 + 3 < H || k0 == count - 1) && first + k0 >= 0 && first + k0 < A.n &&
                           A.margin + j0 + 4 <= A.length && chunk_aligned16(dst);
        if (whole) {
            const float* ya = A.chunks + (size_t)(first + k0) * A.length + A.margin + j0;
            if (k0 == 0 || j0 >= A.fade) {
                if (chunk_aligned16(ya)) {
                    wunet_st4(dst, wunet_ld4(ya));
                    continue;
                }
            } else if (j0 + 4 <= A.fade && first + k0 >= 1) {
                const float* yb = ya - A.length + H;
                if (chunk_aligned16(ya) && chunk_aligned16(yb) && chunk_aligned16(A.ramp + j0)) {
                    const wunet_f4 a = wunet_ld4(ya), b = wunet_ld4(yb), w = wunet_ld4(A.ramp + j0);
                    wunet_f4 o;
#pragma unroll
                    for (int u = 0; u < 4; ++u) o[u] = fmaf(w[u], a[u], (1.0f - w[u]) * b[u]);
                    wunet_st4(dst, o);
                    continue;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long t = t0 + u, g = g0 + u;
            if (t >= T || g < 0 || g >= A.total) continue;
            long long k = t / H;
            if (k > count - 1) k = count - 1;
            float o;
            if (chunk_ola_one(A, first, k, t - k * H, o)) A.out_flat[g] = o;
        }
    }
}
