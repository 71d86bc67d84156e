// Dynamic-LDS layouts of the seven kernels that carve their allocation by hand: one description per kernel, read by the kernel (with
// its template arguments: region pointers and the addressing constants), by the planner (occupancy), by the launcher (the bytes it
// requests) and by the dispatcher of every instantiation (which refuses a request smaller than its layout).  Plain constexpr C++:
// no HIP types, so host-only programs (tools/plan_dump.cpp) and the emulator build read it too.
// A description holds the compile-time geometry as ints and gives every region's offset, in the unit the kernel addresses it by, and
// the total in bytes; what only a launch knows (rowp; ER = the padded rows of the epilogue's table; C8) is an argument.
#pragma once
#include <cstddef>

constexpr size_t WUNET_LDS_PER_CU = 160 * 1024;      // gfx950: LDS of one CU
constexpr size_t WUNET_LDS_OPT_IN = 64 * 1024;       // more dynamic LDS than this must be granted per kernel (hipFuncSetAttribute)

namespace wunet_lds {

constexpr int kWaves = 4;                            // waves of a block (WUNET_WAVES)

// floats of the staged row of the fp32 kernels' x tile: tn positions of a level of L samples are segments of min(L, tn) positions, each
// staged with 8 floats of halo on both sides
constexpr int staged_row(int L, int tn) { return (tn / (L < tn ? L : tn)) * ((L < tn ? L : tn) + 16); }

// ---- conv_mfma_kernel<TAPS, M_REP, N_REP>, floats:  xs [KC][rowp] | ws [M_REP][KC][TAPS][16]
struct ConvMfma {
    int kc, wchunk, mrep;                            // channels per K chunk; floats of one m-tile's K-chunk (240 float4)
    constexpr int ws(int rowp) const { return kc * rowp; }
    constexpr int end(int rowp) const { return ws(rowp) + mrep * wchunk; }
    constexpr size_t bytes(int rowp) const { return (size_t)end(rowp) * sizeof(float); }
};
constexpr ConvMfma conv_mfma(int taps, int mrep) { return {taps == 15 ? 4 : 12, (taps == 15 ? 4 : 12) * taps * 16, mrep}; }
// row stride of the x tile (64 * N_REP positions): the staged row padded to 16 (mod 32)
constexpr int conv_mfma_rowp(int L, int nrep) { int rp = staged_row(L, 64 * nrep); while (rp % 32 != 16) rp += 4; return rp; }

// ---- wgrad_mfma_kernel<TAPS, M_REP, NW, XIT, WSPLIT>, floats:  gs [M_REP*16][GROW] | xs [CIB][rowp]
// (xs is 16-byte aligned: M_REP*16*66*4 is a multiple of 16)
struct WgradMfma {
    int tp, grow, cib, mrep;                         // positions per chunk; g row stride == 2 (mod 32): A fragments conflict free; input channels per block
    constexpr int xs() const { return mrep * 16 * grow; }
    constexpr int end(int rowp) const { return xs() + cib * rowp; }
    constexpr size_t bytes(int rowp) const { return (size_t)end(rowp) * sizeof(float); }
};
constexpr WgradMfma wgrad_mfma(int taps, int mrep, int nw, bool wsplit) { return {64, 64 + 2, wsplit ? 1 : kWaves * nw * (taps == 15 ? 1 : 3), mrep}; }
// row stride of the x rows (chunks of 64 positions): the staged row; 5 taps: padded to 8 (mod 32), the 3 ci rows of an n-tile land on disjoint banks
constexpr int wgrad_mfma_rowp(int taps, int L) { int rp = staged_row(L, 64); if (taps == 5) while (rp % 32 != 8) rp += 4; return rp; }

// ---- wgrad_h3_kernel<TAPS, M_REP, NSEG, TP, BF>, pieces of 16 bytes (8 halfs):
//   gs [hi|lo][GG][GP][8] | xs [hi|lo][XG][XPOS][8] | 8 pieces of slack (the transposed reads of the last rows reach behind the x image)
struct WgradH3 {
    int gp;                                          // TP positions per chunk; plane stride (pieces) of the g_z image, 4 mod 16
    int lseg, swx;                                   // NSEG > 1: L < TP, a chunk is NSEG items, each with its own halo rows
    int xrows;                                       // x rows staged per plane (8 halo + samples + halo)
    int xpos;                                        // plane stride of the x image (4 mod 16)
    int xg, gg, npl;                                 // channel groups of 8 of x / of g_z per block; operand planes: hi (+ lo); BF: one bf16 word per value
    constexpr int xs() const { return npl * gg * gp; }
    constexpr int end() const { return xs() + npl * xg * xpos + 8; }
    constexpr size_t bytes() const { return (size_t)end() * 16; }
};
constexpr WgradH3 wgrad_h3(int taps, int mrep, int nseg, int tp, bool bf)
{
    const int swx = tp / nseg + 16, xrows = nseg == 1 ? tp + 20 : nseg * swx;
    return {tp + 4, tp / nseg, swx, xrows, ((xrows + 11) / 16) * 16 + 4, (taps == 15 ? 2 : 4) * 16 / 8, mrep * 2, bf ? 1 : 2};
}

// ---- wgrad_h3d_kernel<TAPS, M_REP, DB, BF, TP>, pieces of 16 bytes:  [DB ? 2 : 1][ g_z image GPCS | x image XPCS | 8 pieces of slack ]
struct WgradH3d {
    int gp, xpos;                                    // plane strides (pieces), both 4 mod 16
    int xg, gg, npl;
    int gpcs, xpcs;                                  // pieces of the g_z image (rows 128..131 of a plane are never read or written) / of the x image
    int nbuf;
    constexpr int buf() const { return gpcs + xpcs + 8; }
    constexpr int end() const { return nbuf * buf(); }
    constexpr size_t bytes() const { return (size_t)end() * 16; }
};
constexpr WgradH3d wgrad_h3d(int taps, int mrep, bool db, bool bf, int tp)
{
    const int xg = (taps == 15 ? 2 : 4) * 16 / 8, gg = mrep * 2, npl = bf ? 1 : 2;
    return {tp + 4, tp + 20, xg, gg, npl, npl * gg * (tp + 4), npl * xg * (tp + 20), db ? 2 : 1};
}

// ---- conv_h3d_kernel<TAPS, M_REP, NSEG, BF, EVOP, UPT>:
//   pieces of 16 bytes:  xs [hi|lo][4][COLS, de-interleaved][8] | ws [hi|lo][M_REP][TG][4][16][8]
//   floats behind them:  red [4 waves][M_REP * 16][2] statistics hand-over (UPT: room for [4] per row), + 4 maxima
//                        | epi [bias | eval a | eval s][ER]: the epilogue's per-row constants of the un-segmented tiles, once per block
//                          (the eval parts only where they leave the CU its second block: ConvH3Args::epi_eval; UPT - a data gradient
//                          has no bias - and the segmented tiles: no table)
struct ConvH3d {
    int lseg, sw, cols;                              // samples of a segment, with its halo; columns of the tile
    int npl, xp;                                     // planes; pieces of the x tile
    int wpm, wp;                                     // pieces of one m-tile's W run (TG taps x 64) / of the W sub-tile of a stage
    int rw, red_floats;                              // hand-over floats per 16 rows; floats of red = float offset of epi behind it
    bool epi_lds;
    constexpr int ws() const { return xp; }
    constexpr int red() const { return xp + wp; }
    constexpr size_t bytes(int er, int eval) const { return (size_t)red() * 16 + (size_t)(red_floats + (epi_lds ? (eval ? 3 : 1) * er : 0)) * sizeof(float); }
    // blocks of that size a CU holds (launch bounds: two; the 16-segment tile's 96 KB: one) - the table of constants is not counted:
    // its eval part stays in global memory where it would cost the second block
    constexpr int blocks_per_cu() const { return 2 * bytes(0, 0) <= WUNET_LDS_PER_CU ? 2 : 1; }
    constexpr bool eval_table_fits(int er) const { return epi_lds && 2 * bytes(er, 1) <= WUNET_LDS_PER_CU; }
};
constexpr ConvH3d conv_h3d(int mrep, int nseg, bool bf, bool upt)
{
    const int lseg = 256 / nseg, cols = nseg * (lseg + 16), npl = bf ? 1 : 2, rw = upt ? 64 : 32;
    return {lseg, lseg + 16, cols, npl, npl * 4 * cols, 5 * 64, npl * mrep * 5 * 64, rw, kWaves * mrep * rw + 4, nseg == 1 && !upt};
}

// ---- conv_h3u_kernel<M_REP, COPY>:
//   pieces of 16 bytes:  xs0 [2][hi|lo][4][COLS, de-interleaved][8] | ws0 [2][hi|lo][M_REP][TG][4][16][8]
//   floats behind them:  red [4 waves][M_REP * 16][2] statistics hand-over, + 4
//                        | coef [a | s][C8 * 8]: BatchNorm scale / shift of the operand's channels (x the operand scale)
//                        | epi [bias | eval a | eval s][ER]: the epilogue's per-row constants
struct ConvH3u {
    int cols, xp, wpm, wp;                           // columns of a tile; pieces of one x tile (hi + lo), of one m-tile's W run, of one W sub-tile
    int coef;                                        // float offset of coef behind red
    constexpr int ws0() const { return 2 * xp; }
    constexpr int red() const { return 2 * xp + 2 * wp; }
    constexpr int epi(int c8) const { return 2 * c8 * 8; }      // float offset of epi behind coef
    constexpr size_t bytes(int c8, int er) const { return (size_t)red() * 16 + (size_t)(coef + epi(c8) + 3 * er) * sizeof(float); }
};
constexpr ConvH3u conv_h3u(int mrep) { return {272, 2 * 4 * 272, 5 * 64, 2 * mrep * 5 * 64, kWaves * mrep * 32 + 4}; }

// ---- resample_rows_kernel, floats:  hs [ntaps] the filter as it lies in memory | xs [span] the input under one tile of outputs
// A tile is `tile` consecutive outputs of one row, 4 g ng of them with g a multiple of `up`: a thread owns the 4 outputs o, o + g,
// o + 2 g, o + 3 g, which share one phase and so one set of taps (wunet_resample.h).  g ng is about 512, two trips of the block's
// threads, and is taken smaller where `down / up` is so large that the input under the tile would not fit kResampleSpanMax floats.
constexpr int kResampleOut = 4;                      // outputs per thread and trip
constexpr int kResampleSpanMax = 16384;              // floats of xs at the most (64 KiB; with the largest filter 114 KiB of the CU's 160)
struct Resample {
    int g, ng, tile, span, ntaps;
    constexpr int xs() const { return ntaps; }
    constexpr int end() const { return ntaps + span; }
    constexpr size_t bytes() const { return (size_t)end() * sizeof(float); }
};
// floats of input under `tile` outputs: the last output's i_hi minus the first one's, plus the taps of a phase, rounded up
constexpr long long resample_span(long long tile, int up, int down, int ntaps) { return ((tile - 1) * down + (ntaps - 1)) / up + 3; }
constexpr Resample resample(int up, int down, int ntaps)
{
    int k = up < 64 ? 64 / up : 1, ng = 512 / (up * k) > 1 ? 512 / (up * k) : 1;
    while (ng > 1 && resample_span((long long)kResampleOut * up * k * ng, up, down, ntaps) > kResampleSpanMax) --ng;
    while (k > 1 && resample_span((long long)kResampleOut * up * k * ng, up, down, ntaps) > kResampleSpanMax) --k;
    const int g = up * k, tile = kResampleOut * g * ng;
    return {g, ng, tile, (int)resample_span(tile, up, down, ntaps), ntaps};
}

// ---- sos_windows_kernel<S>, doubles first:  es [chunks + 1][2 S + 1] the entry state of every chunk of the tile (row chunks: the
// entry state of the next tile) | ms [2 S][2 S] the chunk-to-chunk transition matrix, row-major;  then floats:  xs [tile + tile / 64]
// the samples of the tile, one float of padding behind every 64.
// A thread owns kSosChunk = 64 consecutive samples, a block kSosTile = 256 * 64: the row of a 16384-sample window and its lead-in is
// two trips, and the scan over the chunks (one dependent 2S x 2S product per chunk, the long pole of the kernel) has 256 steps per
// 16384 samples.  A thread reads its chunk at a stride of 65 floats: lane l on bank (l + k) mod 64, conflict free.  The odd stride of es
// (2 S + 1 doubles) spreads the 2 S stores of a chunk's final state over the banks the same way.  S = 8: 103 KiB, one block per CU.
constexpr int kSosChunk = 64;
constexpr int kSosChunks = 256;                      // chunks of a tile: one per thread (WUNET_THREADS)
constexpr int kSosTile = kSosChunk * kSosChunks;
struct Sos {
    int n;                                           // 2 S, the order of the cascade's state
    constexpr int es_stride() const { return n + 1; }
    constexpr int ms() const { return (kSosChunks + 1) * es_stride(); }                 // (doubles)
    constexpr int xs() const { return 2 * (ms() + n * n); }                             // (floats from here on)
    constexpr int end() const { return xs() + kSosTile + kSosTile / 64; }
    constexpr size_t bytes() const { return (size_t)end() * sizeof(float); }
};
constexpr Sos sos(int sections) { return {2 * sections}; }

// ---- bss_corr_kernel, doubles:  ss [tile + n - 1] the reference under one tile of the row and the n - 1 samples behind it | es the
// estimate over the same span.  Staged as doubles: the inner loop is one double FMA per 8-byte LDS read, no conversion in it.  Thread t
// owns the lags t and t + 256: at every sample it reads ss / es at consecutive addresses across the wave (conflict free) and the tile's
// own sample as a broadcast.  n = 512: 40 KiB, three blocks per CU.
constexpr int kBssTile = 2048;                       // samples of a row a block owns (its segment)
constexpr int kBssMaxFilter = 512;                   // WUNET_BSS_MAX_FILTER: two lags per thread
struct BssCorr {
    int n;                                           // filter length
    constexpr int span() const { return kBssTile + n - 1; }
    constexpr int es() const { return span(); }
    constexpr int end() const { return 2 * span(); }
    constexpr size_t bytes() const { return (size_t)end() * sizeof(double); }
};
constexpr BssCorr bss_corr(int filter_length) { return {filter_length}; }

// ---- bss_solve_kernel, doubles:  rs [512] the autocorrelation | bs [512] the cross-correlation | as [2][512] the prediction
// polynomial of Levinson's recursion, the order before and the order being written (afterwards: the solution c in the first half)
// | red [2 * kWaves] block_sum's hand-over | one double: the estimate's energy.  Sized for the largest filter whatever n is: 16.1 KiB.
struct BssSolve {
    constexpr int bs() const { return kBssMaxFilter; }
    constexpr int as() const { return 2 * kBssMaxFilter; }
    constexpr int red() const { return 4 * kBssMaxFilter; }
    constexpr int energy() const { return red() + 2 * kWaves; }
    constexpr int end() const { return energy() + 1; }
    constexpr size_t bytes() const { return (size_t)end() * sizeof(double); }
};
constexpr BssSolve bss_solve() { return {}; }

}  // namespace wunet_lds
