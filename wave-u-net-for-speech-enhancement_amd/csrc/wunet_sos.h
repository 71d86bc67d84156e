// Cascades of second-order IIR sections over windows of a flat array (include/wunet_hip.h: wunet_sos_windows): the recurrence of
// scipy.signal.sosfilt (transposed direct form II), per row and section
//   o = b0 v + s0;  s0 = b1 v - a1 o + s1;  s1 = b2 v - a2 o
// with the float32 coefficients widened to double, all state and arithmetic in double, each output rounded to float32 once.
//   sos_windows_kernel<S>   one block per row; the row's lead_b + L samples in tiles of wunet_lds::kSosTile
//
// A recurrence is sequential along the row; one thread per row would put (lead + L) S dependent steps on one lane.  The state of the
// cascade is a vector s of n = 2 S doubles, and one sample maps it affinely, s' = A s + x u.  So does a chunk of C samples: with f the
// state that the chunk leaves when it is entered at rest and M = A^C,  s_out = M s_in + f  - not approximately: it is the same
// linear map, regrouped.  That is what runs here, per tile:
//   load    the tile's samples into LDS, coalesced dwords, masked (what lies outside the source is 0.0f, never addressed)
//   pass 1  thread c runs the cascade over chunk c from rest and stores f_c                       (C S dependent section steps)
//   scan    lanes r < n of wave 0: e_(c+1)[r] = f_c[r] + sum_k M[r][k] e_c[k], chunk after chunk  (one n-term dot product per chunk)
//   pass 2  thread c runs chunk c again from its true entry state e_c and writes the float32 outputs over its samples in LDS
//   store   the outputs at j >= 0 to global memory, coalesced dwords; e_0 of the next tile = the scan's last value
// M is built once per row: lane i < n runs C zero-input steps from the unit state i, which gives column i.  The dependent chain of a
// tile is about 2 C S section steps + one dot product per chunk instead of C S chunks-per-tile section steps.
// Rounding: pass 2 inside a chunk is the plain recurrence on its entry state.  The entry states differ from the plain recurrence's by
// the rounding of one n x n product per chunk in place of C steps of it (tests/sos_cases.py: within a few units of what
// scipy's own double recurrence is away from the exact result, for the near-unit poles of a 20 Hz high-pass too).
// No atomics, every output written by one thread, every sum in a fixed order: bit-identical run to run.  Everything ragged (the row
// table, the coefficients) is read from device memory.  A row with non-finite coefficients fills only its own row.
// The geometry (C, tile, the LDS regions) has one definition, wunet_lds::sos.
#pragma once
#include "wunet_dev.h"
#include "wunet_lds.h"

struct SosArgs {
    const float* flat;
    long long total;
    const long long* rows;       // [batch][4]: window start, item start, circular length, phase
    const float* coefs;          // [batch][S][5]: b0 b1 b2 a1 a2
    int lead, length;
    float* out;                  // [batch][1][length]
};

// one sample through the cascade: v in, the last section's o out; s = (s0, s1) of every section
template <int S>
__device__ __forceinline__ double sos_step(const double (&k)[S][5], double (&s)[2 * S], double v)
{
#pragma unroll
    for (int q = 0; q < S; ++q) {
        const double o = k[q][0] * v + s[2 * q];
        s[2 * q] = k[q][1] * v - k[q][3] * o + s[2 * q + 1];
        s[2 * q + 1] = k[q][2] * v - k[q][4] * o;
        v = o;
    }
    return v;
}

// grid = batch blocks of WUNET_THREADS (== wunet_lds::kSosChunks) threads.
template <int S>
static __global__ __launch_bounds__(WUNET_THREADS) void sos_windows_kernel(SosArgs A)
{
    constexpr int N = 2 * S, C = wunet_lds::kSosChunk, TILE = wunet_lds::kSosTile;
    constexpr wunet_lds::Sos lay = wunet_lds::sos(S);
    constexpr int ES = lay.es_stride();
    WUNET_DYN_SMEM(smem);
    double* es = reinterpret_cast<double*>(smem);
    double* ms = es + lay.ms();
    float* xs = smem + lay.xs();
    const int b = blockIdx.x, tid = threadIdx.x, L = A.length;
    float* out = A.out + (size_t)b * L;

    // ---- the row's source after clamping.  Linear: x[j] = base[j] for j >= -lead_b (lead_b <= ws - is: never in front of the item).
    // Circular: x[j] = base[(ph + j) mod nl].  Nothing outside [0, total) is ever addressed.
    const long long* r = A.rows + 4 * (size_t)b;
    long long ws = r[0], is = r[1], nl = r[2], ph = r[3];
    const bool circular = nl >= 1;
    int lead = A.lead;
    const float* base;
    if (!circular) {
        if (ws < 0) ws = 0;
        if (ws > A.total - L) ws = A.total - L;
        if (is < 0) is = 0;
        if (is > ws) is = ws;
        if (ws - is < (long long)lead) lead = (int)(ws - is);
        base = A.flat + ws;
        nl = 0; ph = 0;
    } else {
        // (bounded first, so that is + nl cannot overflow on a corrupt table: wunet_mix.h's mix_row)
        if (nl > A.total) nl = A.total;
        if (is > A.total) is = A.total;
        if (is < -A.total) is = -A.total;
        const long long lo = is < 0 ? 0 : is, hi = is + nl < A.total ? is + nl : A.total;
        nl = hi > lo ? hi - lo : 0;
        if (nl == 0) {                                   // nothing is left of the item: a row of zeros
            for (int j = tid; j < L; j += WUNET_THREADS) out[j] = 0.0f;
            return;
        }
        ph %= nl;
        if (ph < 0) ph += nl;
        base = A.flat + lo;
    }
    const int total_n = lead + L;                        // samples the filter runs over; sample q is x[q - lead]

    double k[S][5];
    {
        const float* cf = A.coefs + (size_t)b * S * 5;
#pragma unroll
        for (int q = 0; q < S; ++q)
#pragma unroll
            for (int u = 0; u < 5; ++u) k[q][u] = (double)cf[q * 5 + u];
    }
    // ---- M = (one-step transition)^C, column tid: C zero-input steps from the unit state tid.  e_0 of the first tile: at rest.
    if (tid < N) {
        double s[N];
#pragma unroll
        for (int i = 0; i < N; ++i) s[i] = i == tid ? 1.0 : 0.0;
        for (int t = 0; t < C; ++t) sos_step<S>(k, s, 0.0);
#pragma unroll
        for (int i = 0; i < N; ++i) ms[i * N + tid] = s[i];
        es[tid] = 0.0;
    }

    // position inside the circular item of this thread's first sample of the first tile, and its step from trip to trip of the load
    long long kpos = 0, kstep = 0;
    if (circular) {
        kpos = (ph + (long long)tid - (long long)lead) % nl;
        if (kpos < 0) kpos += nl;
        kstep = (long long)WUNET_THREADS % nl;
    }

    for (int q0 = 0; q0 < total_n; q0 += TILE) {
        const int cnt = total_n - q0 < TILE ? total_n - q0 : TILE;      // samples of this tile
        const int nch = (cnt + C - 1) / C;                              // its chunks; all but the row's last one are full
        // ---- load (the barrier at the end of the trip before has ended every read of xs)
        for (int i = tid; i < cnt; i += WUNET_THREADS) {
            float v;
            if (circular) {
                v = base[kpos];
                kpos += kstep;
                if (kpos >= nl) kpos -= nl;
            } else {
                v = base[(long long)(q0 + i) - lead];
            }
            xs[i + (i >> 6)] = v;
        }
        // (a tile that is not the last is full, a multiple of WUNET_THREADS: every thread has advanced kpos by the same trips)
        __syncthreads();
        // ---- pass 1: the state that chunk tid leaves when it is entered at rest
        const int c0 = tid * C, clen = cnt - c0 < C ? cnt - c0 : C;     // (clen <= 0: no chunk for this thread)
        float* xc = xs + c0 + tid;
        if (tid < nch) {
            double s[N];
#pragma unroll
            for (int i = 0; i < N; ++i) s[i] = 0.0;
            for (int t = 0; t < clen; ++t) sos_step<S>(k, s, (double)xc[t]);
#pragma unroll
            for (int i = 0; i < N; ++i) es[(tid + 1) * ES + i] = s[i];
        }
        __syncthreads();
        // ---- scan: es[c + 1] = M es[c] + f_c.  One barrier per chunk; lanes tid < N hold row tid of M in registers.
        {
            double m[N];
            if (tid < N) {
#pragma unroll
                for (int i = 0; i < N; ++i) m[i] = ms[tid * N + i];
            }
            for (int c = 0; c < nch; ++c) {
                if (tid < N) {
                    double acc = es[(c + 1) * ES + tid];
#pragma unroll
                    for (int i = 0; i < N; ++i) acc += m[i] * es[c * ES + i];
                    es[(c + 1) * ES + tid] = acc;
                }
                __syncthreads();
            }
        }
        // ---- pass 2: chunk tid from its true entry state; the float32 outputs replace the samples
        if (tid < nch) {
            double s[N];
#pragma unroll
            for (int i = 0; i < N; ++i) s[i] = es[tid * ES + i];
            for (int t = 0; t < clen; ++t) xc[t] = (float)sos_step<S>(k, s, (double)xc[t]);
        }
        __syncthreads();
        // ---- store what lies at j >= 0; the next tile starts from the scan's last state
        for (int i = tid; i < cnt; i += WUNET_THREADS) {
            const int j = q0 + i - lead;
            if (j >= 0) out[j] = xs[i + (i >> 6)];
        }
        if (tid < N) es[tid] = es[nch * ES + tid];
        __syncthreads();
    }
}
