// What the MFMA waves of conv_h3d_kernel (wunet_h3d.h) and conv_h3u_kernel (wunet_h3u.h) both run - ONE copy: the two kernels give
// bit-identical results because they share these fragments, this MFMA order per accumulator and this epilogue arithmetic.
//   WUNET_H3_LOAD_A, WUNET_H3_PASS                          the stage's arithmetic: A-fragment read, one pass-major MFMA pass
//   WUNET_H3_EPI_FILL                                       the epilogue's per-row constants into LDS
//   WUNET_H3_ROW_BIAS, WUNET_H3_ROWS, WUNET_H3_EPILOGUE     the row epilogue and its dispatch
//   wunet_h3_stats_row                                      the statistics row of a tile
// All but the last are textual macros that take every operand by name (nothing is captured from the kernel): as functions they change
// conv_h3d_kernel's register allocation, and that kernel has instantiations at 256 VGPRs that answer with spills or a lost wave per
// SIMD (which piece did what: DESIGN.md section 3, profiles/conv_shared_mma_ab.txt).  A macro expands to the text the kernels held
// before, so every instantiation keeps its instruction stream.  No ablation bits in here: each kernel keeps its own around the calls.
#pragma once
#include "wunet_h3.h"

// A fragments of tap tl_ of the W sub-tile ws_ [hi|lo][M_REP][TG][4][16][8] -> ah_[M_REP], al_[M_REP] (BF: one plane, al_ untouched);
// aoff_ = the lane's (quarter, row) inside a fragment
#define WUNET_H3_LOAD_A(M_REP_, TG_, BF_, ws_, aoff_, tl_, ah_, al_)                                              \
    _Pragma("unroll") for (int mt = 0; mt < (M_REP_); ++mt) {                                                     \
        ah_[mt] = wunet_ldh8((ws_) + ((mt * (TG_) + (tl_)) * 64) * 8 + (aoff_));                                  \
        if (!(BF_)) al_[mt] = wunet_ldh8((ws_) + (((M_REP_) + mt) * (TG_) + (tl_)) * 64 * 8 + (aoff_));           \
    }
// One pass of tap tl_ over the M_REP x 4 accumulators acc_: WHICH_ 0 = lo*hi, 1 = hi*lo, 2 = hi*hi (BF: only pass 2 exists).  Pass-major
// issue puts 4 M_REP independent MFMAs between two on the same accumulator; per accumulator the order of the products never changes.
// B fragment (n-tile nt, tap tl_) = fh_ / fl_[tl_ + nt].
#define WUNET_H3_PASS(WHICH_, M_REP_, BF_, acc_, ah_, al_, fh_, fl_, tl_)                                         \
    _Pragma("unroll") for (int mt = 0; mt < (M_REP_); ++mt)                                                       \
        _Pragma("unroll") for (int nt = 0; nt < 4; ++nt) {                                                        \
            if (BF_) { if ((WHICH_) == 2) acc_[mt][nt] = wunet_mfma16b(ah_[mt], fh_[(tl_) + nt], acc_[mt][nt]); } \
            else if ((WHICH_) == 0) acc_[mt][nt] = wunet_mfma16h(al_[mt], fh_[(tl_) + nt], acc_[mt][nt]);         \
            else if ((WHICH_) == 1) acc_[mt][nt] = wunet_mfma16h(ah_[mt], fl_[(tl_) + nt], acc_[mt][nt]);         \
            else acc_[mt][nt] = wunet_mfma16h(ah_[mt], fh_[(tl_) + nt], acc_[mt][nt]);                            \
        }

// The epilogue's per-row constants epi_ = [bias | eval a | eval s][ER_] in LDS, once per block, by every thread of it (ER_ = the rows of
// all row blocks; rows beyond Cout: 0; no bias unless usebias_; the eval parts only where evpart_ - they may not fit otherwise - and
// zeros unless evon_)
#define WUNET_H3_EPI_FILL(A_, epi_, ER_, usebias_, evpart_, evon_, tid_, nthreads_)                               \
    for (int c = (tid_); c < (ER_); c += (nthreads_)) {                                                           \
        const bool in = c < (A_).Cout;                                                                            \
        (epi_)[c] = (in && (A_).bias && (usebias_)) ? (A_).bias[c] : 0.0f;                                        \
        if (evpart_) {                                                                                            \
            (epi_)[(ER_) + c] = (in && (evon_)) ? (A_).ev_a[c] : 0.0f;                                            \
            (epi_)[2 * (ER_) + c] = (in && (evon_)) ? (A_).ev_s[c] : 0.0f;                                        \
        }                                                                                                         \
    }

// The rows of one work item, for the lane (q_ = lane >> 4, i16_ = lane & 15) of MFMA wave wave_: rows (mt0_ + mt) * 16 + q_ * 4 + r, row
// (mt, r) at prow_ + (mt * 16 + r) * L (uniform strides: no 64-bit multiply per row).  STATS_: Sigma, Sigma^2 of the bias-free conv per
// row, per wave, into red_ [4 waves][M_REP * 16][2]; GUARD_: rows beyond Cout exist, or the lane's batch item does not (live_); EVAL_: the
// activation bound of eval mode into amax_ (its a / s from the LDS table where evtab_); EVOP_: the activation at the lane's two even
// samples goes to EVOPM_(mt, ye) - conv_h3d_kernel's store of the consumer's operand; nostore_: ablation builds without the stores.
#define WUNET_H3_NO_EVOP(mt_, ye_)
#define WUNET_H3_ROWS(STATS_, GUARD_, EVAL_, EVOP_, EVOPM_, M_REP_, A_, acc_, bvs_, inv12_, prow_, mt0_, q_, i16_, wave_, live_, nostore_, epi_, ER_, evtab_, red_, amax_) \
    float eas[M_REP_][4], ess[M_REP_][4];                                                                         \
    if (EVAL_) {                                                  /* one batch of loads, like the biases */      \
        _Pragma("unroll") for (int mt = 0; mt < (M_REP_); ++mt)                                                   \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                       \
                const int co = ((mt0_) + mt) * 16 + (q_) * 4 + r;                                                 \
                eas[mt][r] = (evtab_) ? (epi_)[(ER_) + co] : co < (A_).Cout ? (A_).ev_a[co] : 0.0f;               \
                ess[mt][r] = (evtab_) ? (epi_)[2 * (ER_) + co] : co < (A_).Cout ? (A_).ev_s[co] : 0.0f;           \
            }                                                                                                     \
    }                                                                                                             \
    _Pragma("unroll") for (int mt = 0; mt < (M_REP_); ++mt) {                                                     \
        float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};                                         \
        float ye[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};                                            \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                           \
            const int co = ((mt0_) + mt) * 16 + (q_) * 4 + r;                                                     \
            const float bv = bvs_[mt][r];                                                                         \
            wunet_f4 o;                                                                                           \
            _Pragma("unroll") for (int nt = 0; nt < 4; ++nt) {                                                    \
                const float vv = acc_[mt][nt][r] * (inv12_);                                                      \
                if (STATS_) { s1[r] += vv; s2[r] = fmaf(vv, vv, s2[r]); }                                         \
                o[nt] = vv + bv;                                                                                  \
            }                                                                                                     \
            if ((!(GUARD_) || (co < (A_).Cout && (live_))) && (!(nostore_) || o[0] == 123.456f)) {                \
                wunet_st4((prow_) + (size_t)(mt * 16 + r) * (A_).L, o);                                           \
                if (EVAL_) {                                                                                      \
                    const float ea = eas[mt][r], es = ess[mt][r];                                                 \
                    _Pragma("unroll") for (int nt = 0; nt < 4; ++nt) amax_ = fmaxf(amax_, fabsf(ea * o[nt] + es)); \
                    if (EVOP_) { ye[0][r] = wunet_lrelu(ea * o[0] + es); ye[1][r] = wunet_lrelu(ea * o[2] + es); } \
                }                                                                                                 \
            }                                                                                                     \
        }                                                                                                         \
        if ((EVOP_) && (EVAL_)) { EVOPM_(mt, ye) }                                                                \
        if (STATS_) {                                                                                             \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                       \
                s1[r] = wunet_row16_sum(s1[r]);                                                                   \
                s2[r] = wunet_row16_sum(s2[r]);                                                                   \
                if ((i16_) == 0) {                            /* per-wave sums of row mt*16 + q*4 + r -> LDS */   \
                    float* rp = (red_) + (((wave_) * (M_REP_) + mt) * 16 + (q_) * 4 + r) * 2;                     \
                    rp[0] = s1[r];                                                                                \
                    rp[1] = s2[r];                                                                                \
                }                                                                                                 \
            }                                                                                                     \
        }                                                                                                         \
    }
// The rows' biases bvs_[M_REP][4] in ONE batch of loads, from the LDS table (EPI_LDS_) or, where usebias_, from global memory: loaded
// row by row where they are used, each load was waited for with vmcnt(0) - i.e. together with the previous row's store - and the
// 4*M_REP serialised round trips were a third of a shallow layer's block time (phase stamps, tools/conv_bench.py --trace)
#define WUNET_H3_ROW_BIAS(M_REP_, EPI_LDS_, A_, bvs_, mt0_, q_, usebias_, epi_)                                   \
    _Pragma("unroll") for (int mt = 0; mt < (M_REP_); ++mt)                                                       \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                           \
            const int co = ((mt0_) + mt) * 16 + (q_) * 4 + r;                                                     \
            bvs_[mt][r] = (EPI_LDS_) ? (epi_)[co] : ((usebias_) && co < (A_).Cout) ? (A_).bias[co] : 0.0f;        \
        }
// The row epilogue of one work item: copies of the row loop behind uniform branches - the un-guarded, statistics-free one (data
// gradients, K splits) is half the instructions; full_: no row / item of the tile lies outside the tensor.
#define WUNET_H3_EPILOGUE(EVOP_, EVOPM_, M_REP_, A_, acc_, bvs, inv12_, prow_, mt0_, q_, i16_, wave_, live_, nostore_, epi_, ER_, evtab_, red_, amax_, want_stats_, full_) \
    {                                                                                                             \
        if ((A_).xrows) { WUNET_H3_ROWS(false, true, true, EVOP_, EVOPM_, M_REP_, A_, acc_, bvs, inv12_, prow_, mt0_, q_, i16_, wave_, live_, nostore_, epi_, ER_, evtab_, red_, amax_) } \
        else if (want_stats_) {                                                                                   \
            if (full_) { WUNET_H3_ROWS(true, false, false, false, WUNET_H3_NO_EVOP, M_REP_, A_, acc_, bvs, inv12_, prow_, mt0_, q_, i16_, wave_, live_, nostore_, epi_, ER_, false, red_, amax_) } \
            else { WUNET_H3_ROWS(true, true, false, false, WUNET_H3_NO_EVOP, M_REP_, A_, acc_, bvs, inv12_, prow_, mt0_, q_, i16_, wave_, live_, nostore_, epi_, ER_, false, red_, amax_) } \
        } else {                                                                                                  \
            if (full_) { WUNET_H3_ROWS(false, false, false, false, WUNET_H3_NO_EVOP, M_REP_, A_, acc_, bvs, inv12_, prow_, mt0_, q_, i16_, wave_, live_, nostore_, epi_, ER_, false, red_, amax_) } \
            else { WUNET_H3_ROWS(false, true, false, false, WUNET_H3_NO_EVOP, M_REP_, A_, acc_, bvs, inv12_, prow_, mt0_, q_, i16_, wave_, live_, nostore_, epi_, ER_, false, red_, amax_) } \
        }                                                                                                         \
    }

// One statistics row per tile (256 positions), behind a barrier: the four MFMA waves' sums in `red` are added in wave order by the
// block's first M_REP * 16 threads - one row each
template <int M_REP>
__device__ __forceinline__ void wunet_h3_stats_row(const float* red, int tid, int mt0, int Cout, float* stats, int ntiles, int tile)
{
    if (tid < M_REP * 16) {
        const float* rp = red + tid * 2;
        float t1 = 0.0f, t2 = 0.0f;
#pragma unroll
        for (int w = 0; w < WUNET_WAVES; ++w) {
            t1 += rp[w * M_REP * 32];
            t2 += rp[w * M_REP * 32 + 1];
        }
        const int co = mt0 * 16 + tid;
        if (co < Cout) {
            float* stp = stats + ((size_t)co * ntiles + tile) * 2;
            stp[0] = t1;
            stp[1] = t2;
        }
    }
}
