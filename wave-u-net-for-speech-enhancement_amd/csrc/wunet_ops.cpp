// Loss, fused Adam, window crops, profiler read-out and the single-op entry points (tests / tools) of libwunet_hip.so
// (see wunet_host.h).
#include "wunet_host.h"
#include "wunet_elementwise.h"
#include "wunet_h3_elem.h"
#include "wunet_adam.h"
#include "wunet_loss_mean.h"
#include "wunet_loss_rows.h"
#include "wunet_stft.h"
#include "wunet_cspec.h"
#include "wunet_mel.h"
#include "wunet_stoi.h"
#include "wunet_estoi.h"
#include "wunet_mix.h"
#include "wunet_reverb.h"
#include "wunet_chunks.h"
#include "wunet_resample.h"
#include "wunet_sos.h"
#include "wunet_bss.h"

using namespace wunet_host;

// the ones and zeros that stand in for BatchNorm's scale and shift in the single-op entry points (op_conv_split_common, op_wgrad_split_common)
static __global__ __launch_bounds__(WUNET_THREADS) void fill_kernel(float* p, size_t n, float v)
{
    for (size_t i = (size_t)blockIdx.x * WUNET_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * WUNET_THREADS) p[i] = v;
}

extern "C" {

size_t wunet_loss_scratch_bytes(void) { return 256 * sizeof(double); }

int wunet_loss_forward(int kind, const float* clean, const float* enhanced, size_t n, float* loss_out, void* scratch, void* stream)
{
    if (kind < 0 || kind > 2 || !clean || !enhanced || !loss_out || !scratch || n == 0) return fail(WUNET_E_ARG, "bad loss argument");
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = capped_blocks(n, WUNET_THREADS * 8, 256);
    WUNET_LAUNCH(loss_partial_kernel, dim3(blocks), dim3(WUNET_THREADS), 0, st, kind, clean, enhanced, n, (double*)scratch);
    WUNET_CHECK_LAUNCH();
    WUNET_LAUNCH(loss_final_kernel, dim3(1), dim3(WUNET_THREADS), 0, st, (const double*)scratch, (int)blocks, n, loss_out);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

int wunet_loss_backward(int kind, const float* clean, const float* enhanced, const float* grad_loss, size_t n, float* grad_enhanced, void* stream)
{
    if (kind < 0 || kind > 2 || !clean || !enhanced || !grad_loss || !grad_enhanced || n == 0) return fail(WUNET_E_ARG, "bad loss argument");
    hipStream_t st = (hipStream_t)stream;
    WUNET_LAUNCH(loss_bwd_kernel, dim3(capped_blocks(n, WUNET_THREADS * 4, 2048)), dim3(WUNET_THREADS), 0, st, kind, clean, enhanced, grad_loss, n, grad_enhanced);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

// ---------------------------------------------------------------------------- the (row, piece) grids of the row losses and the mixer
// Pieces per row and samples per piece for `rows` rows of `len` samples: about want_blocks blocks in all, so one long row still fills
// the device, but never less than min_piece samples per block - many rows get one piece each.  plen is a multiple of 4 (every piece of
// an aligned row starts aligned) and ppr is recomputed from it: no piece is empty (row_piece in wunet_row_piece.h).
static void row_pieces(size_t rows, size_t len, size_t want_blocks, size_t min_piece, size_t& ppr, size_t& plen)
{
    size_t want = (want_blocks + rows - 1) / rows;
    const size_t most = (len + min_piece - 1) / min_piece;
    if (want > most) want = most;
    if (want < 1) want = 1;
    plen = (((len + want - 1) / want) + 3) & ~(size_t)3;
    ppr = (len + plen - 1) / plen;
}

// ---------------------------------------------------------------------------- row losses (SI-SDR / SNR per utterance)
#define WUNET_ROWS_BLOCKS 512
#define WUNET_ROWS_MIN_PIECE 4096        // 4 trips of 16-byte loads per thread

static int loss_rows_shape_check(size_t rows, size_t row_len)
{
    if (rows == 0 || row_len == 0) return fail(WUNET_E_ARG, "row loss: rows and row_len must be > 0 (got %zu x %zu)", rows, row_len);
    if (rows >= (1ull << 30) || row_len >= (1ull << 40)) return fail(WUNET_E_ARG, "row loss: shape too large (%zu x %zu)", rows, row_len);
    return 0;
}

size_t wunet_loss_rows_scratch_bytes(size_t rows, size_t row_len)
{
    if (rows == 0 || row_len == 0) return 0;
    size_t ppr, plen;
    row_pieces(rows, row_len, WUNET_ROWS_BLOCKS, WUNET_ROWS_MIN_PIECE, ppr, plen);
    return rows * ppr * WUNET_ROWS_SUMS * sizeof(double);
}

int wunet_loss_rows_forward(int kind, int zero_mean, double eps, const float* clean, const float* enhanced, size_t rows, size_t row_len,
                            float* loss_out, float* per_row_db, double* coefs, void* scratch, void* stream)
{
    if (kind != WUNET_LOSS_SI_SDR && kind != WUNET_LOSS_SNR) return fail(WUNET_E_ARG, "row loss: unknown kind %d (WUNET_LOSS_SI_SDR or WUNET_LOSS_SNR)", kind);
    if (loss_rows_shape_check(rows, row_len)) return WUNET_E_ARG;
    if (!clean || !enhanced || !loss_out || !scratch) return fail(WUNET_E_ARG, "row loss: null argument");
    if (!(eps >= 0.0) || eps > 1.7976931348623157e308) return fail(WUNET_E_ARG, "row loss: eps must be finite and >= 0 (got %g)", eps);
    hipStream_t st = (hipStream_t)stream;
    size_t ppr, plen;
    row_pieces(rows, row_len, WUNET_ROWS_BLOCKS, WUNET_ROWS_MIN_PIECE, ppr, plen);
    WUNET_LAUNCH(loss_rows_partial_kernel, dim3((unsigned)(rows * ppr)), dim3(WUNET_THREADS), 0, st, kind, clean, enhanced, row_len, (unsigned)ppr,
                 plen, (double*)scratch);
    WUNET_CHECK_LAUNCH();
    LossRowsFinalArgs A{};
    A.part = (const double*)scratch; A.rows = rows; A.T = row_len; A.ppr = (unsigned)ppr;
    A.group = 1;
    while (A.group < 64 && (size_t)A.group < ppr) A.group <<= 1;
    A.kind = kind; A.zero_mean = zero_mean != 0; A.eps = eps; A.loss = loss_out; A.per_row = per_row_db; A.coefs = coefs;
    WUNET_LAUNCH(loss_rows_final_kernel, dim3(1), dim3(WUNET_THREADS), 0, st, A);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

int wunet_loss_rows_backward(int kind, const float* clean, const float* enhanced, const double* coefs, const float* grad_loss, size_t rows,
                             size_t row_len, float* grad_enhanced, void* stream)
{
    if (kind != WUNET_LOSS_SI_SDR && kind != WUNET_LOSS_SNR) return fail(WUNET_E_ARG, "row loss: unknown kind %d (WUNET_LOSS_SI_SDR or WUNET_LOSS_SNR)", kind);
    if (loss_rows_shape_check(rows, row_len)) return WUNET_E_ARG;
    if (!clean || !enhanced || !coefs || !grad_loss || !grad_enhanced) return fail(WUNET_E_ARG, "row loss: null argument");
    hipStream_t st = (hipStream_t)stream;
    size_t ppr, plen;
    row_pieces(rows, row_len, WUNET_ROWS_BLOCKS, WUNET_ROWS_MIN_PIECE, ppr, plen);
    WUNET_LAUNCH(loss_rows_bwd_kernel, dim3((unsigned)(rows * ppr)), dim3(WUNET_THREADS), 0, st, kind, clean, enhanced, coefs, grad_loss, rows, row_len,
                 (unsigned)ppr, plen, grad_enhanced);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

// ---------------------------------------------------------------------------- multi-resolution STFT loss (wunet_stft.h)
namespace {
struct StftShape { size_t rows, T; int N, H; unsigned M, F; int BP, bins, k0, k1; unsigned mtiles; };      // (rows, T, N, H: the call's own)

// every constraint of one resolution on (rows, T); fills the derived sizes.  T == 0 (the basis calls): the checks that need the waveform are skipped.
int stft_shape(size_t rows, size_t T, int N, int H, int W, StftShape& s)
{
    s.rows = rows; s.T = T; s.N = N; s.H = H;
    if (N < 16 || N > 4096 || N % 16) return fail(WUNET_E_ARG, "stft: n_fft must be a multiple of 16 in 16 .. 4096 (got %d)", N);
    if (W < 1 || W > N) return fail(WUNET_E_ARG, "stft: win_length must be in 1 .. n_fft (got %d, n_fft %d)", W, N);
    s.bins = N / 2 + 1;
    s.BP = (s.bins + WUNET_STFT_BN - 1) / WUNET_STFT_BN * WUNET_STFT_BN;
    const int left = (N - W) / 2;
    s.k0 = left / WUNET_STFT_KT * WUNET_STFT_KT;
    s.k1 = (left + W + WUNET_STFT_KT - 1) / WUNET_STFT_KT * WUNET_STFT_KT;
    if (T == 0) return 0;
    if (H < 1 || H > N) return fail(WUNET_E_ARG, "stft: hop must be in 1 .. n_fft (got %d, n_fft %d)", H, N);
    if (rows == 0) return fail(WUNET_E_ARG, "stft: rows must be > 0");
    if ((size_t)(N / 2) + 1 > T) return fail(WUNET_E_ARG, "stft: reflect padding needs n_fft / 2 <= T - 1 (n_fft %d, T %zu)", N, T);
    if (T >= (1ull << 30) || rows >= (1ull << 30) || rows * T >= (1ull << 38)) return fail(WUNET_E_ARG, "stft: shape too large (%zu x %zu)", rows, T);
    const size_t F = 1 + T / (size_t)H, M = rows * F;
    if (M >= (1ull << 31) - WUNET_STFT_FM) return fail(WUNET_E_ARG, "stft: too many frames (%zu rows x %zu)", rows, F);
    s.F = (unsigned)F; s.M = (unsigned)M;
    s.mtiles = (unsigned)((M + WUNET_STFT_FM - 1) / WUNET_STFT_FM);
    return 0;
}
inline size_t stft_nparts(const StftShape& s) { return (size_t)s.mtiles * (size_t)(s.BP / WUNET_STFT_BN); }

// ---- one host path for the STFT loss, the compressed spectral loss (wunet_cspec.h) and the mel loss (wunet_mel.h); `what` ("stft" /
// "cspec" / "mel") starts the messages
// the resolution of one call (stft_shape's messages say "stft" for all); what == nullptr: a size query, an empty row is 0 without a message
int spectral_shape(const char* what, size_t rows, size_t row_len, int n_fft, int hop, int win_length, StftShape& s)
{
    if (row_len == 0) return what ? fail(WUNET_E_ARG, "%s: row_len must be > 0", what) : WUNET_E_ARG;
    return stft_shape(rows, row_len, n_fft, hop, win_length, s);
}
int mel_filters(int n_mels)
{
    return n_mels < 1 || n_mels > WUNET_MEL_MAX ? fail(WUNET_E_ARG, "mel: n_mels must be in 1 .. %d (got %d)", WUNET_MEL_MAX, n_mels) : 0;
}
// the blocks of mel_proj_kernel: WUNET_MEL_FM frames each
inline unsigned mel_blocks(const StftShape& s) { return (s.M + WUNET_MEL_FM - 1) / WUNET_MEL_FM; }
// the forward's partials (`fwd` bytes), or with `bwd` the adjoint GEMM's M x n_fft floats where those are more
inline size_t spectral_scratch(const StftShape& s, size_t fwd, int bwd) { const size_t b = bwd ? (size_t)s.M * s.N * sizeof(float) : 0; return b > fwd ? b : fwd; }
// StftFwdArgs of one resolution (CspecFwdArgs carries one as .S); returns the forward's grid.  (extern "C++", here and on the two templates
// below: this whole file is one extern "C" block, which allows neither a template nor a C++ class as a result)
extern "C++" dim3 fill_fwd_args(StftFwdArgs& A, const StftShape& s, const float* clean, const float* enhanced, double clamp, const float* basis,
                                void* scratch, float* saved, float* mag_out)
{
    A.c = clean; A.e = enhanced; A.basis = basis; A.T = s.T; A.M = s.M; A.F = s.F; A.N = s.N; A.H = s.H; A.BP = s.BP; A.bins = s.bins;
    A.k0 = s.k0; A.k1 = s.k1; A.clamp = (float)clamp; A.part = (double*)scratch; A.saved = saved; A.mag_out = mag_out;
    return dim3(s.mtiles, (unsigned)(s.BP / WUNET_STFT_BN));
}
// part / nparts / count of StftFinalArgs or CspecFinalArgs: one entry per resolution.  n_mels (the mel loss): one partial per block
// of mel_proj_kernel, and the mean runs over the mel cells, not the bins
extern "C++" template <class Args>
int fill_final_args(Args& A, const char* what, int n_res, const void* const* scratch, size_t rows, size_t row_len, const int* n_fft, const int* hop,
                    const int* n_mels = nullptr)
{
    for (int i = 0; i < n_res; ++i) {
        StftShape s{};
        if (spectral_shape(what, rows, row_len, n_fft[i], hop[i], 1, s)) return WUNET_E_ARG;
        if (!scratch[i]) return fail(WUNET_E_ARG, "%s: null scratch of resolution %d", what, i);
        if (n_mels && mel_filters(n_mels[i])) return WUNET_E_ARG;
        A.part[i] = (const double*)scratch[i];
        A.nparts[i] = n_mels ? mel_blocks(s) : (unsigned)stft_nparts(s);
        A.count[i] = (double)s.M * (double)(n_mels ? n_mels[i] : s.bins);
    }
    return 0;
}
// the adjoint-GEMM fields of StftBwdArgs or CspecBwdArgs and the profiler's record of `kernel`, which reads `planes` saved planes
extern "C++" template <class Args>
void fill_adjoint_args(Args& B, const char* kernel, int planes, const StftShape& s, const float* saved, const double* coefs, const float* basis,
                       double clamp, void* scratch, hipStream_t st)
{
    B.saved = saved; B.coefs = coefs; B.basis = basis; B.M = s.M; B.N = s.N; B.BP = s.BP; B.bins = s.bins; B.k0 = s.k0; B.k1 = s.k1;
    B.clamp = (float)clamp; B.scratch = (float*)scratch;
    B.ktiles = (unsigned)((s.k1 - s.k0 + WUNET_STFT_BWN - 1) / WUNET_STFT_BWN);           // (at most 32; mtiles < 2^25)
    prof_begin(st, kernel, 2.0 * s.M * (s.k1 - s.k0) * 2.0 * s.BP, 4.0 * ((double)planes * s.M * s.BP + (double)(s.k1 - s.k0) * (2.0 * s.BP + s.M)));
}
// the overlap-add of the adjoint GEMM's frames into grad_enhanced: the tail of both backwards
int launch_stft_ola(const StftShape& s, const void* scratch, const float* grad_loss, float* grad_enhanced, int accumulate, hipStream_t st)
{
    StftOlaArgs O{};
    O.scratch = (const float*)scratch; O.gl = grad_loss; O.g = grad_enhanced; O.T = s.T; O.total = s.rows * s.T; O.F = s.F;
    O.N = s.N; O.H = s.H; O.k0 = s.k0; O.k1 = s.k1; O.accumulate = accumulate != 0;
    prof_begin(st, "stft_ola_kernel", 0.0, 4.0 * ((double)s.M * (s.k1 - s.k0) + (accumulate ? 2.0 : 1.0) * s.rows * s.T));
    WUNET_LAUNCH(stft_ola_kernel, dim3((unsigned)((O.total + WUNET_THREADS - 1) / WUNET_THREADS)), dim3(WUNET_THREADS), 0, st, O);
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}
inline size_t cspec_fwd_bytes(const StftShape& s) { return stft_nparts(s) * 2 * sizeof(double); }
inline size_t cspec_saved(const StftShape& s) { return (size_t)WUNET_CSPEC_PLANES * s.M * s.BP * sizeof(float); }
// the mel loss's forward scratch: one partial (two doubles) per block of mel_proj_kernel, then the planes S_e, S_c [M][BP] (mel_spec_kernel -> mel_proj_kernel)
inline size_t mel_part_bytes(const StftShape& s) { return (size_t)mel_blocks(s) * 2 * sizeof(double); }
inline size_t mel_fwd_bytes(const StftShape& s) { return mel_part_bytes(s) + (size_t)2 * s.M * s.BP * sizeof(float); }
inline int mel_padded(int n_mels) { return (n_mels + 15) & ~15; }
inline size_t mel_saved(const StftShape& s, int n_mels) { return MelLayout(s.M, s.BP, mel_padded(n_mels)).floats() * sizeof(float); }
// power, clamp and floor of one call; `loss`: the pair (clamp and floor > 0), else the spectrogram alone (>= 0)
int mel_knobs(int power, double clamp, double floor, bool loss)
{
    if (power != 1 && power != 2) return fail(WUNET_E_ARG, "mel: power must be 1 or 2 (got %d)", power);
    if (!(loss ? clamp > 0.0 : clamp >= 0.0) || clamp > 3.0e38) return fail(WUNET_E_ARG, "mel: clamp must be finite and %s 0 (got %g)", loss ? ">" : ">=", clamp);
    if (!(loss ? floor > 0.0 : floor >= 0.0) || floor > 3.0e38) return fail(WUNET_E_ARG, "mel: floor must be finite and %s 0 (got %g)", loss ? ">" : ">=", floor);
    return 0;
}
int cspec_knobs(double compress, double clamp)
{
    if (!(compress > 0.0) || compress > 1.0) return fail(WUNET_E_ARG, "cspec: compress must be in (0, 1] (got %g)", compress);
    if (!(clamp > 0.0) || clamp > 3.0e38) return fail(WUNET_E_ARG, "cspec: clamp must be finite and > 0 (got %g)", clamp);
    return 0;
}
}  // namespace

size_t wunet_stft_basis_bytes(int n_fft)
{
    StftShape s{};
    if (stft_shape(0, 0, n_fft, 1, 1, s)) return 0;
    return (size_t)n_fft * 2 * s.BP * sizeof(float);
}

int wunet_stft_basis(int n_fft, int win_length, float* basis, void* stream)
{
    StftShape s{};
    if (stft_shape(0, 0, n_fft, 1, win_length, s)) return WUNET_E_ARG;
    if (!basis || ((size_t)basis & 15)) return fail(WUNET_E_ARG, "stft: the basis needs a 16-byte aligned buffer");
    WUNET_LAUNCH(stft_basis_kernel, dim3((unsigned)((2 * s.BP + WUNET_THREADS - 1) / WUNET_THREADS), (unsigned)n_fft), dim3(WUNET_THREADS), 0,
                 (hipStream_t)stream, n_fft, win_length, s.BP, basis);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

size_t wunet_stft_scratch_bytes(size_t rows, size_t row_len, int n_fft, int hop, int with_backward)
{
    StftShape s{};
    return spectral_shape(nullptr, rows, row_len, n_fft, hop, 1, s) ? 0 : spectral_scratch(s, stft_nparts(s) * 3 * sizeof(double), with_backward);
}

size_t wunet_stft_saved_bytes(size_t rows, size_t row_len, int n_fft, int hop)
{
    StftShape s{};
    return spectral_shape(nullptr, rows, row_len, n_fft, hop, 1, s) ? 0 : (size_t)3 * s.M * s.BP * sizeof(float);
}

int wunet_stft_forward(const float* clean, const float* enhanced, size_t rows, size_t row_len, int n_fft, int hop, int win_length,
                       double clamp, const float* basis, void* scratch, float* saved, float* mag_out, void* stream)
{
    StftShape s{};
    if (spectral_shape("stft", rows, row_len, n_fft, hop, win_length, s)) return WUNET_E_ARG;
    if (!enhanced || !basis || ((size_t)basis & 15)) return fail(WUNET_E_ARG, "stft: null argument (or a basis that is not 16-byte aligned)");
    if (clean) {
        if (!(clamp > 0.0) || clamp > 3.0e38) return fail(WUNET_E_ARG, "stft: clamp must be finite and > 0 (got %g)", clamp);
        if (!scratch) return fail(WUNET_E_ARG, "stft: the loss forward needs wunet_stft_scratch_bytes of scratch");
    } else {
        if (!(clamp >= 0.0) || clamp > 3.0e38) return fail(WUNET_E_ARG, "stft: clamp must be finite and >= 0 (got %g)", clamp);
        if (!mag_out || saved) return fail(WUNET_E_ARG, "stft: without `clean` the call writes mag_out only");
    }
    StftFwdArgs A{};
    const dim3 grid = fill_fwd_args(A, s, clean, enhanced, clamp, basis, scratch, saved, mag_out);
    // (profiler: 2 flops x frames x window support x 2 BP columns per signal; the waveforms and the basis once, the saved spectra)
    prof_begin((hipStream_t)stream, clean ? "stft_fwd_kernel<pair>" : "stft_fwd_kernel<one>", (clean ? 2.0 : 1.0) * 2.0 * s.M * (s.k1 - s.k0) * 2.0 * s.BP,
               4.0 * ((clean ? 2.0 : 1.0) * rows * row_len + (double)(s.k1 - s.k0) * 2.0 * s.BP + (saved ? 3.0 * s.M * s.BP : 0.0)));
    if (clean) {
        WUNET_LAUNCH(stft_fwd_kernel<true>, grid, dim3(WUNET_THREADS), 0, (hipStream_t)stream, A);
    } else {
        WUNET_LAUNCH(stft_fwd_kernel<false>, grid, dim3(WUNET_THREADS), 0, (hipStream_t)stream, A);
    }
    prof_end((hipStream_t)stream);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

int wunet_stft_finalize(int n_res, const void* const* scratch, size_t rows, size_t row_len, const int* n_fft, const int* hop,
                        double sc_weight, double mag_weight, float* loss_out, double* coefs, void* stream)
{
    if (n_res < 1 || n_res > WUNET_STFT_MAX_RES) return fail(WUNET_E_ARG, "stft: 1 .. %d resolutions per call (got %d)", WUNET_STFT_MAX_RES, n_res);
    if (!scratch || !n_fft || !hop || !loss_out) return fail(WUNET_E_ARG, "stft: null argument");
    if (!(sc_weight == sc_weight) || !(mag_weight == mag_weight)) return fail(WUNET_E_ARG, "stft: a weight is NaN");
    StftFinalArgs A{};
    if (fill_final_args(A, "stft", n_res, scratch, rows, row_len, n_fft, hop)) return WUNET_E_ARG;
    A.n_res = n_res; A.w_sc = sc_weight; A.w_mag = mag_weight; A.loss = loss_out; A.coefs = coefs;
    WUNET_LAUNCH(stft_final_kernel, dim3(1), dim3(WUNET_THREADS), 0, (hipStream_t)stream, A);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

int wunet_stft_backward(const float* saved, const double* coefs, const float* grad_loss, size_t rows, size_t row_len, int n_fft, int hop,
                        int win_length, double clamp, const float* basis, void* scratch, float* grad_enhanced, int accumulate, void* stream)
{
    StftShape s{};
    if (spectral_shape("stft", rows, row_len, n_fft, hop, win_length, s)) return WUNET_E_ARG;
    if (!saved || !coefs || !grad_loss || !basis || !scratch || !grad_enhanced || ((size_t)basis & 15))
        return fail(WUNET_E_ARG, "stft: null argument (or a basis that is not 16-byte aligned)");
    if (!(clamp > 0.0) || clamp > 3.0e38) return fail(WUNET_E_ARG, "stft: clamp must be finite and > 0 (got %g)", clamp);
    hipStream_t st = (hipStream_t)stream;
    StftBwdArgs B{};
    fill_adjoint_args(B, "stft_bwd_kernel", 3, s, saved, coefs, basis, clamp, scratch, st);
    WUNET_LAUNCH(stft_bwd_kernel, dim3(B.ktiles * s.mtiles), dim3(WUNET_THREADS), 0, st, B);
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    return launch_stft_ola(s, scratch, grad_loss, grad_enhanced, accumulate, st);
}

// ---------------------------------------------------------------------------- compressed spectral loss (wunet_cspec.h)
size_t wunet_cspec_scratch_bytes(size_t rows, size_t row_len, int n_fft, int hop, int with_backward)
{
    StftShape s{};
    return spectral_shape(nullptr, rows, row_len, n_fft, hop, 1, s) ? 0 : spectral_scratch(s, cspec_fwd_bytes(s), with_backward);
}

size_t wunet_cspec_saved_bytes(size_t rows, size_t row_len, int n_fft, int hop)
{
    StftShape s{};
    return spectral_shape(nullptr, rows, row_len, n_fft, hop, 1, s) ? 0 : cspec_saved(s);
}

int wunet_cspec_forward(const float* clean, const float* enhanced, size_t rows, size_t row_len, int n_fft, int hop, int win_length,
                        double compress, double clamp, const float* basis, void* scratch, size_t scratch_bytes, float* saved,
                        size_t saved_bytes, void* stream)
{
    StftShape s{};
    if (spectral_shape("cspec", rows, row_len, n_fft, hop, win_length, s) || cspec_knobs(compress, clamp)) return WUNET_E_ARG;
    if (!clean || !enhanced || !basis || ((size_t)basis & 15)) return fail(WUNET_E_ARG, "cspec: null argument (or a basis that is not 16-byte aligned)");
    if (!scratch || scratch_bytes < cspec_fwd_bytes(s))
        return fail(WUNET_E_ARG, "cspec: the forward needs %zu bytes of scratch for this resolution (got %zu)", cspec_fwd_bytes(s), scratch_bytes);
    if (saved ? saved_bytes != cspec_saved(s) : saved_bytes != 0)
        return fail(WUNET_E_ARG, "cspec: saved must be the %zu bytes of wunet_cspec_saved_bytes for this resolution, or NULL and 0 (got %zu)",
                    cspec_saved(s), saved_bytes);
    CspecFwdArgs C{};
    const dim3 grid = fill_fwd_args(C.S, s, clean, enhanced, clamp, basis, scratch, saved, nullptr);
    C.hs = 0.5 * (compress - 1.0);
    prof_begin((hipStream_t)stream, "cspec_fwd_kernel", 2.0 * 2.0 * s.M * (s.k1 - s.k0) * 2.0 * s.BP,
               4.0 * (2.0 * rows * row_len + (double)(s.k1 - s.k0) * 2.0 * s.BP + (saved ? (double)WUNET_CSPEC_PLANES * s.M * s.BP : 0.0)));
    WUNET_LAUNCH(cspec_fwd_kernel, grid, dim3(WUNET_THREADS), 0, (hipStream_t)stream, C);
    prof_end((hipStream_t)stream);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

int wunet_cspec_finalize(int n_res, const void* const* scratch, size_t rows, size_t row_len, const int* n_fft, const int* hop,
                         double complex_weight, float* loss_out, double* coefs, void* stream)
{
    if (n_res < 1 || n_res > WUNET_STFT_MAX_RES) return fail(WUNET_E_ARG, "cspec: 1 .. %d resolutions per call (got %d)", WUNET_STFT_MAX_RES, n_res);
    if (!scratch || !n_fft || !hop || !loss_out) return fail(WUNET_E_ARG, "cspec: null argument");
    if (!(complex_weight >= 0.0) || complex_weight > 1.0) return fail(WUNET_E_ARG, "cspec: complex_weight must be in [0, 1] (got %g)", complex_weight);
    CspecFinalArgs A{};
    if (fill_final_args(A, "cspec", n_res, scratch, rows, row_len, n_fft, hop)) return WUNET_E_ARG;
    A.n_res = n_res; A.w0 = 1.0 - complex_weight; A.w1 = complex_weight; A.loss = loss_out; A.coefs = coefs;
    WUNET_LAUNCH(cspec_final_kernel, dim3(1), dim3(WUNET_THREADS), 0, (hipStream_t)stream, A);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

int wunet_cspec_backward(const float* saved, size_t saved_bytes, const double* coefs, const float* grad_loss, size_t rows, size_t row_len,
                         int n_fft, int hop, int win_length, double compress, double clamp, const float* basis, void* scratch,
                         size_t scratch_bytes, float* grad_enhanced, int accumulate, void* stream)
{
    StftShape s{};
    if (spectral_shape("cspec", rows, row_len, n_fft, hop, win_length, s) || cspec_knobs(compress, clamp)) return WUNET_E_ARG;
    if (!saved || !coefs || !grad_loss || !basis || !grad_enhanced || ((size_t)basis & 15))
        return fail(WUNET_E_ARG, "cspec: null argument (or a basis that is not 16-byte aligned)");
    if (saved_bytes != cspec_saved(s))
        return fail(WUNET_E_ARG, "cspec: saved must be the %zu bytes of wunet_cspec_saved_bytes for this resolution (got %zu)", cspec_saved(s), saved_bytes);
    if (!scratch || scratch_bytes < spectral_scratch(s, 0, 1))
        return fail(WUNET_E_ARG, "cspec: the backward needs %zu bytes of scratch for this resolution (got %zu)", spectral_scratch(s, 0, 1), scratch_bytes);
    hipStream_t st = (hipStream_t)stream;
    CspecBwdArgs B{};
    B.compress = compress; B.hs = 0.5 * (compress - 1.0);
    fill_adjoint_args(B, "cspec_bwd_kernel", WUNET_CSPEC_PLANES, s, saved, coefs, basis, clamp, scratch, st);
    WUNET_LAUNCH(cspec_bwd_kernel, dim3(B.ktiles * s.mtiles), dim3(WUNET_THREADS), 0, st, B);
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    return launch_stft_ola(s, scratch, grad_loss, grad_enhanced, accumulate, st);
}

// ---------------------------------------------------------------------------- multi-scale log-mel loss (wunet_mel.h)
size_t wunet_mel_scratch_bytes(size_t rows, size_t row_len, int n_fft, int hop, int with_backward)
{
    StftShape s{};
    return spectral_shape(nullptr, rows, row_len, n_fft, hop, 1, s) ? 0 : spectral_scratch(s, mel_fwd_bytes(s), with_backward);
}

size_t wunet_mel_saved_bytes(size_t rows, size_t row_len, int n_fft, int hop, int n_mels)
{
    StftShape s{};
    return spectral_shape(nullptr, rows, row_len, n_fft, hop, 1, s) || mel_filters(n_mels) ? 0 : mel_saved(s, n_mels);
}

int wunet_mel_forward(const float* clean, const float* enhanced, size_t rows, size_t row_len, int n_fft, int hop, int win_length, int n_mels,
                      const float* filt, int power, double clamp, double floor, const float* basis, void* scratch, size_t scratch_bytes,
                      float* saved, size_t saved_bytes, float* mel_out, void* stream)
{
    StftShape s{};
    if (spectral_shape("mel", rows, row_len, n_fft, hop, win_length, s) || mel_filters(n_mels) || mel_knobs(power, clamp, floor, clean != nullptr))
        return WUNET_E_ARG;
    if (!enhanced || !basis || !filt || (((size_t)basis | (size_t)filt) & 15))
        return fail(WUNET_E_ARG, "mel: null argument (or a basis or a filterbank that is not 16-byte aligned)");
    if (!scratch || ((size_t)scratch & 15) || scratch_bytes < mel_fwd_bytes(s))
        return fail(WUNET_E_ARG, "mel: the forward needs %zu bytes of 16-byte aligned scratch for this resolution (got %zu)", mel_fwd_bytes(s), scratch_bytes);
    if (clean) {
        if (saved ? saved_bytes != mel_saved(s, n_mels) || ((size_t)saved & 15) : saved_bytes != 0)
            return fail(WUNET_E_ARG, "mel: saved must be the %zu bytes (16-byte aligned) of wunet_mel_saved_bytes for this resolution, or NULL and 0 (got %zu)",
                        mel_saved(s, n_mels), saved_bytes);
        if (mel_out) return fail(WUNET_E_ARG, "mel: mel_out belongs to the call without `clean`");
    } else if (!mel_out || saved || saved_bytes) {
        return fail(WUNET_E_ARG, "mel: without `clean` the call writes mel_out only (saved NULL and 0)");
    }
    hipStream_t st = (hipStream_t)stream;
    const double nsig = clean ? 2.0 : 1.0;
    MelSpecArgs C{};
    const dim3 grid = fill_fwd_args(C.S, s, clean, enhanced, clamp, basis, nullptr, saved, nullptr);
    C.spec = (float*)((char*)scratch + mel_part_bytes(s)); C.power = power;
    prof_begin(st, clean ? "mel_spec_kernel<pair>" : "mel_spec_kernel<one>", nsig * 2.0 * s.M * (s.k1 - s.k0) * 2.0 * s.BP,
               4.0 * (nsig * rows * row_len + (double)(s.k1 - s.k0) * 2.0 * s.BP + (nsig + (saved ? 2.0 : 0.0)) * s.M * s.BP));
    if (clean) {
        WUNET_LAUNCH(mel_spec_kernel<true>, grid, dim3(WUNET_THREADS), 0, st, C);
    } else {
        WUNET_LAUNCH(mel_spec_kernel<false>, grid, dim3(WUNET_THREADS), 0, st, C);
    }
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    MelProjArgs P{};
    P.spec = C.spec; P.filt = filt; P.M = s.M; P.BP = s.BP; P.bins = s.bins; P.n_mels = n_mels; P.MP = mel_padded(n_mels); P.floor = floor;
    P.part = (double*)scratch; P.saved = saved; P.mel_out = mel_out;
    prof_begin(st, clean ? "mel_proj_kernel<pair>" : "mel_proj_kernel<one>", nsig * 2.0 * s.M * s.bins * n_mels,
               4.0 * (nsig * s.M * s.BP + (double)n_mels * s.BP + (saved ? 2.0 * s.M * P.MP : 0.0) + (mel_out ? (double)s.M * n_mels : 0.0)));
    if (clean) {
        WUNET_LAUNCH(mel_proj_kernel<true>, dim3(mel_blocks(s)), dim3(WUNET_THREADS), 0, st, P);
    } else {
        WUNET_LAUNCH(mel_proj_kernel<false>, dim3(mel_blocks(s)), dim3(WUNET_THREADS), 0, st, P);
    }
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

int wunet_mel_finalize(int n_res, const void* const* scratch, size_t rows, size_t row_len, const int* n_fft, const int* hop, const int* n_mels,
                       double log_weight, double lin_weight, float* loss_out, double* coefs, void* stream)
{
    if (n_res < 1 || n_res > WUNET_STFT_MAX_RES) return fail(WUNET_E_ARG, "mel: 1 .. %d resolutions per call (got %d)", WUNET_STFT_MAX_RES, n_res);
    if (!scratch || !n_fft || !hop || !n_mels || !loss_out) return fail(WUNET_E_ARG, "mel: null argument");
    if (!(log_weight >= 0.0) || !(lin_weight >= 0.0) || log_weight > 1.0e300 || lin_weight > 1.0e300 || log_weight + lin_weight == 0.0)
        return fail(WUNET_E_ARG, "mel: log_weight and lin_weight must be finite and >= 0, not both 0 (got %g, %g)", log_weight, lin_weight);
    CspecFinalArgs A{};
    if (fill_final_args(A, "mel", n_res, scratch, rows, row_len, n_fft, hop, n_mels)) return WUNET_E_ARG;
    A.n_res = n_res; A.w0 = log_weight; A.w1 = lin_weight; A.loss = loss_out; A.coefs = coefs;
    WUNET_LAUNCH(cspec_final_kernel, dim3(1), dim3(WUNET_THREADS), 0, (hipStream_t)stream, A);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

int wunet_mel_backward(float* saved, size_t saved_bytes, const double* coefs, const float* grad_loss, size_t rows, size_t row_len, int n_fft,
                       int hop, int win_length, int n_mels, const float* filt, int power, double clamp, double floor, const float* basis,
                       void* scratch, size_t scratch_bytes, float* grad_enhanced, int accumulate, void* stream)
{
    StftShape s{};
    if (spectral_shape("mel", rows, row_len, n_fft, hop, win_length, s) || mel_filters(n_mels) || mel_knobs(power, clamp, floor, true)) return WUNET_E_ARG;
    if (!saved || !coefs || !grad_loss || !basis || !filt || !grad_enhanced || (((size_t)basis | (size_t)filt | (size_t)saved) & 15))
        return fail(WUNET_E_ARG, "mel: null argument (or a basis, a filterbank or a saved buffer that is not 16-byte aligned)");
    if (saved_bytes != mel_saved(s, n_mels))
        return fail(WUNET_E_ARG, "mel: saved must be the %zu bytes of wunet_mel_saved_bytes for this resolution (got %zu)", mel_saved(s, n_mels), saved_bytes);
    if (!scratch || scratch_bytes < spectral_scratch(s, 0, 1))
        return fail(WUNET_E_ARG, "mel: the backward needs %zu bytes of scratch for this resolution (got %zu)", spectral_scratch(s, 0, 1), scratch_bytes);
    hipStream_t st = (hipStream_t)stream;
    MelProjBwdArgs P{};
    P.saved = saved; P.coefs = coefs; P.filt = filt; P.M = s.M; P.BP = s.BP; P.n_mels = n_mels; P.MP = mel_padded(n_mels); P.floor = floor;
    prof_begin(st, "mel_proj_bwd_kernel", 2.0 * s.M * s.BP * n_mels, 4.0 * (2.0 * s.M * P.MP + (double)n_mels * s.BP + (double)s.M * s.BP));
    WUNET_LAUNCH(mel_proj_bwd_kernel, dim3(s.mtiles, (unsigned)((s.BP + WUNET_STFT_BWN - 1) / WUNET_STFT_BWN)), dim3(WUNET_THREADS), 0, st, P);
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    MelBwdArgs B{};
    B.power = power;
    fill_adjoint_args(B, "mel_bwd_kernel", WUNET_MEL_PLANES, s, saved, coefs, basis, clamp, scratch, st);
    WUNET_LAUNCH(mel_bwd_kernel, dim3(B.ktiles * s.mtiles), dim3(WUNET_THREADS), 0, st, B);
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    return launch_stft_ola(s, scratch, grad_loss, grad_enhanced, accumulate, st);
}

// ---------------------------------------------------------------------------- STOI and ESTOI per row (wunet_stoi.h, wunet_estoi.h)
// One host path for both: `extended` picks the segment stage (estoi_segment_kernel; in the backward estoi_segment_bwd_kernel +
// estoi_gather_kernel) and the backward's scratch for the segments' gradient blocks - nothing else forks.
namespace {
struct StoiShape {
    int p, q, L;            // 10 kHz = fs p / q; L = 0 without resampling
    size_t Tr;              // samples of a row at 10 kHz
    unsigned F0, Fmax, M, nblk;
    size_t o_nk, o_kept, o_energy, o_res, o_pw, o_part, bytes;   // byte offsets inside the scratch
};

// the resampler of one sample rate: p, q and the filter half length L = ceil(52 / (28.714 fc / 10)), fc = 1 / (2 max(p, q))
int stoi_rate(int fs, StoiShape& s)
{
    if (fs <= 0) return fail(WUNET_E_ARG, "stoi: the sample rate must be > 0 (got %d)", fs);
    int a = WUNET_STOI_FS, b = fs;
    while (b) { const int t = a % b; a = b; b = t; }
    s.p = WUNET_STOI_FS / a; s.q = fs / a; s.L = 0;
    if (fs == WUNET_STOI_FS) return 0;
    const double fc = 1.0 / (2.0 * (double)(s.p > s.q ? s.p : s.q));
    const double L = std::ceil(52.0 / (28.714 * fc / 10.0));
    if (2.0 * L + 1.0 > (double)WUNET_STOI_MAX_TAPS)
        return fail(WUNET_E_ARG, "stoi: %d Hz is %d / %d of 10 kHz and needs %.0f filter taps; at most %d are supported (max(p, q) <= 56)", fs, s.q,
                    s.p, 2.0 * L + 1.0, WUNET_STOI_MAX_TAPS);
    s.L = (int)L;
    return 0;
}

int stoi_shape(size_t rows, size_t T, int fs, StoiShape& s)
{
    if (stoi_rate(fs, s)) return WUNET_E_ARG;
    if (rows == 0) return fail(WUNET_E_ARG, "stoi: rows must be > 0");
    if (rows > 65535) return fail(WUNET_E_ARG, "stoi: at most 65535 rows per call (got %zu)", rows);       // (a grid's y)
    if (T >= (1ull << 30) || rows * T >= (1ull << 36)) return fail(WUNET_E_ARG, "stoi: shape too large (%zu x %zu)", rows, T);
    s.Tr = (T * (size_t)s.p + (size_t)s.q - 1) / (size_t)s.q;
    if (s.Tr >= (1ull << 30) || rows * s.Tr >= (1ull << 36)) return fail(WUNET_E_ARG, "stoi: shape too large at 10 kHz (%zu x %zu)", rows, s.Tr);
    s.F0 = s.Tr > WUNET_STOI_N ? (unsigned)((s.Tr - WUNET_STOI_N + WUNET_STOI_HOP - 1) / WUNET_STOI_HOP) : 0u;
    s.Fmax = s.F0 > 0 ? s.F0 - 1 : 0u;
    if ((size_t)rows * s.Fmax >= (1ull << 31) - WUNET_STFT_FM) return fail(WUNET_E_ARG, "stoi: too many frames (%zu rows x %u)", rows, s.Fmax);
    s.M = (unsigned)(rows * s.Fmax);
    s.nblk = s.Fmax >= WUNET_STOI_SEG ? (s.Fmax - WUNET_STOI_SEG + 1 + WUNET_STOI_SB - 1) / WUNET_STOI_SB : 0u;
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o += (bytes + 15) & ~(size_t)15; return at; };
    s.o_nk = take(rows * sizeof(int));
    s.o_kept = take(rows * s.F0 * sizeof(int));
    s.o_energy = take(rows * s.F0 * sizeof(double));
    s.o_res = take(s.L ? 2 * rows * s.Tr * sizeof(float) : 0);
    s.o_pw = take(s.nblk ? (size_t)2 * s.M * WUNET_STOI_BP * sizeof(float) : 0);
    s.o_part = take(rows * s.nblk * sizeof(double));
    s.bytes = o;
    return 0;
}
}  // namespace

size_t wunet_stoi_tables_bytes(int fs)
{
    StoiShape s{};
    if (stoi_rate(fs, s)) return 0;
    return ((size_t)WUNET_STOI_TAB_TAPS + (s.L ? 2 * (size_t)s.L + 1 : 0) + 3) / 4 * 4 * sizeof(float);
}

int wunet_stoi_tables_build(int fs, const float* taps, size_t n_taps, float* tables, void* stream)
{
    StoiShape s{};
    if (stoi_rate(fs, s)) return WUNET_E_ARG;
    const size_t want = s.L ? 2 * (size_t)s.L + 1 : 0;
    if (n_taps != want) return fail(WUNET_E_ARG, "stoi: %d Hz needs %zu resampler taps (got %zu)", fs, want, n_taps);
    if (!tables || ((size_t)tables & 15) || (want && !taps)) return fail(WUNET_E_ARG, "stoi: null argument (or tables that are not 16-byte aligned)");
    const unsigned grid = WUNET_STOI_N + 1 + (unsigned)((want + WUNET_THREADS - 1) / WUNET_THREADS);
    WUNET_LAUNCH(stoi_tables_kernel, dim3(grid), dim3(WUNET_THREADS), 0, (hipStream_t)stream, taps, (unsigned)want, tables);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

size_t wunet_stoi_scratch_bytes(size_t rows, size_t row_len, int fs)
{
    StoiShape s{};
    if (stoi_shape(rows, row_len, fs, s)) return 0;
    return s.bytes;
}

namespace {
struct StoiBuffers {
    int *nk, *kept, *inv;   // inv: nullptr for the metric
    double* energy;
    float* res;             // [2][rows][Tr], used where the rate is not 10 kHz
    float* pw;              // [2][M][BP]
    float* reim;            // nullptr for the metric: the spectrum kernel then keeps the powers only
    double* part;
};

// resampling, mask, spectra and segment sums of both entry points: everything but the final kernel
int stoi_enqueue(const float* clean, const float* estimate, size_t rows, size_t row_len, const StoiShape& s, const float* tables, const StoiBuffers& B,
                 bool extended, hipStream_t st)
{
    const float* w = tables + WUNET_STOI_TAB_W;
    const float* x[2] = {clean, estimate};
    if (s.L && s.Tr > 0) {
        StoiResampleArgs R{};
        R.in[0] = clean; R.in[1] = estimate; R.taps = tables + WUNET_STOI_TAB_TAPS; R.out = B.res;
        R.T = row_len; R.Tr = s.Tr; R.rows = rows; R.p = s.p; R.q = s.q; R.L = s.L;
        const unsigned per = WUNET_THREADS * WUNET_STOI_RPT;
        prof_begin(st, "stoi_resample_kernel", 2.0 * 2.0 * rows * s.Tr * ((2.0 * s.L + 1.0) / s.p), 4.0 * 2.0 * rows * (row_len + s.Tr));
        WUNET_LAUNCH(stoi_resample_kernel, dim3((unsigned)((s.Tr + per - 1) / per), (unsigned)rows, 2), dim3(WUNET_THREADS), 0, st, R);
        prof_end(st);
        WUNET_CHECK_LAUNCH();
        x[0] = R.out; x[1] = R.out + rows * s.Tr;
    }
    if (s.F0 > 0) {
        StoiMaskArgs K{};
        K.x = x[0]; K.w = w; K.Tr = s.Tr; K.F0 = s.F0; K.energy = B.energy; K.kept = B.kept; K.nk = B.nk; K.inv = B.inv;
        WUNET_LAUNCH(stoi_mask_kernel, dim3((unsigned)rows), dim3(WUNET_THREADS), 0, st, K);
        WUNET_CHECK_LAUNCH();
    }
    if (s.nblk > 0) {       // (fewer than 30 frames at the most: no row has a segment, the final kernel alone writes 1e-5)
        StoiSpecArgs P{};
        P.x[0] = x[0]; P.x[1] = x[1]; P.basis = tables; P.w = w; P.kept = B.kept; P.nk = B.nk; P.Tr = s.Tr; P.M = s.M; P.Fmax = s.Fmax; P.F0 = s.F0;
        P.pw = B.pw; P.reim = B.reim;
        const unsigned mtiles = (s.M + WUNET_STFT_FM - 1) / WUNET_STFT_FM;
        const dim3 grid(mtiles, WUNET_STOI_BP / WUNET_STFT_BN);
        // (profiler: 2 flops x frames x 256 x 2 BP columns per signal, at the largest frame count; the signals once, the powers written)
        if (B.reim) {
            prof_begin(st, "stoi_spec_kernel<save>", 2.0 * 2.0 * s.M * WUNET_STOI_N * 2.0 * WUNET_STOI_BP, 4.0 * (2.0 * rows * s.Tr + 4.0 * s.M * WUNET_STOI_BP));
            WUNET_LAUNCH(stoi_spec_kernel<true>, grid, dim3(WUNET_THREADS), 0, st, P);
        } else {
            prof_begin(st, "stoi_spec_kernel", 2.0 * 2.0 * s.M * WUNET_STOI_N * 2.0 * WUNET_STOI_BP, 4.0 * (2.0 * rows * s.Tr + 2.0 * s.M * WUNET_STOI_BP));
            WUNET_LAUNCH(stoi_spec_kernel<false>, grid, dim3(WUNET_THREADS), 0, st, P);
        }
        prof_end(st);
        WUNET_CHECK_LAUNCH();
        StoiSegArgs G{};
        G.pw = P.pw; G.nk = B.nk; G.M = s.M; G.Fmax = s.Fmax; G.nblk = s.nblk; G.clip = 1.0 + std::pow(10.0, 15.0 / 20.0); G.part = B.part;
        prof_begin(st, extended ? "estoi_segment_kernel" : "stoi_segment_kernel", 0.0, 4.0 * 2.0 * s.M * WUNET_STOI_BP);
        if (extended)
            WUNET_LAUNCH(estoi_segment_kernel, dim3(s.nblk, (unsigned)rows), dim3(WUNET_THREADS), 0, st, G);
        else
            WUNET_LAUNCH(stoi_segment_kernel, dim3(s.nblk, (unsigned)rows), dim3(WUNET_THREADS), 0, st, G);
        prof_end(st);
        WUNET_CHECK_LAUNCH();
    }
    return WUNET_OK;
}

// the loss: what the backward needs (saved) and the scratch of either direction, byte offsets
struct StoiLossShape {
    StoiShape s;
    size_t v_nk, v_kept, v_inv, v_pw, v_reim, saved_bytes;
    size_t f_energy, f_res, f_part, f_score;            // forward
    size_t b_gr, b_fg, b_g10k, b_blk;                   // backward; b_blk: the segments' gradient blocks (ESTOI)
    size_t scratch_bytes;
};

int stoi_loss_shape(size_t rows, size_t T, int fs, bool extended, StoiLossShape& l)
{
    if (stoi_shape(rows, T, fs, l.s)) return WUNET_E_ARG;
    const StoiShape& s = l.s;
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o += (bytes + 15) & ~(size_t)15; return at; };
    const size_t spectra = s.nblk ? (size_t)2 * s.M * WUNET_STOI_BP * sizeof(float) : 0;
    l.v_nk = take(rows * sizeof(int));
    l.v_kept = take(rows * s.F0 * sizeof(int));
    l.v_inv = take(rows * s.F0 * sizeof(int));
    l.v_pw = take(spectra);
    l.v_reim = take(spectra);
    l.saved_bytes = o;
    o = 0;
    l.f_energy = take(rows * s.F0 * sizeof(double));
    l.f_res = take(s.L ? 2 * rows * s.Tr * sizeof(float) : 0);
    l.f_part = take(rows * s.nblk * sizeof(double));
    l.f_score = take(rows * sizeof(double));
    const size_t fwd = o;
    o = 0;
    l.b_gr = take(s.nblk ? (size_t)s.M * WUNET_STOI_BANDS * sizeof(double) : 0);
    l.b_fg = take(s.nblk ? (size_t)s.M * WUNET_STOI_N * sizeof(float) : 0);
    l.b_g10k = take(s.L ? rows * s.Tr * sizeof(float) : 0);
    l.b_blk = take(extended && s.nblk ? rows * (size_t)(s.Fmax - WUNET_STOI_SEG + 1) * WUNET_ESTOI_BLK * sizeof(double) : 0);
    l.scratch_bytes = o > fwd ? o : fwd;
    return 0;
}

// the bodies of the wunet_stoi_* / wunet_estoi_* entry points below
int stoi_forward(bool extended, const float* clean, const float* estimate, size_t rows, size_t row_len, int fs, const float* tables, void* scratch,
                 float* out, int* frames_out, void* stream)
{
    StoiShape s{};
    if (stoi_shape(rows, row_len, fs, s)) return WUNET_E_ARG;
    if (!clean || !estimate || !tables || !scratch || !out || ((size_t)tables & 15) || ((size_t)scratch & 15))
        return fail(WUNET_E_ARG, "stoi: null argument (or tables / scratch that are not 16-byte aligned)");
    hipStream_t st = (hipStream_t)stream;
    char* sc = (char*)scratch;
    StoiBuffers B{};
    B.nk = (int*)(sc + s.o_nk); B.kept = (int*)(sc + s.o_kept); B.energy = (double*)(sc + s.o_energy); B.res = (float*)(sc + s.o_res);
    B.pw = (float*)(sc + s.o_pw); B.part = (double*)(sc + s.o_part);
    if (const int rc = stoi_enqueue(clean, estimate, rows, row_len, s, tables, B, extended, st)) return rc;
    WUNET_LAUNCH(stoi_final_kernel, dim3((unsigned)rows), dim3(WUNET_THREADS), 0, st, (const double*)B.part, (const int*)(s.F0 > 0 ? B.nk : nullptr), s.nblk,
                 out, frames_out, (double*)nullptr);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

size_t stoi_loss_bytes(bool extended, bool saved, size_t rows, size_t row_len, int fs)
{
    StoiLossShape l{};
    if (stoi_loss_shape(rows, row_len, fs, extended, l)) return 0;
    return saved ? l.saved_bytes : l.scratch_bytes;
}

int stoi_loss_forward(bool extended, const float* clean, const float* estimate, size_t rows, size_t row_len, int fs, const float* tables, void* scratch,
                      void* saved, float* loss_out, float* per_row_out, int* frames_out, void* stream)
{
    StoiLossShape l{};
    if (stoi_loss_shape(rows, row_len, fs, extended, l)) return WUNET_E_ARG;
    if (!clean || !estimate || !tables || !scratch || !saved || !loss_out || ((size_t)tables & 15) || ((size_t)scratch & 15) || ((size_t)saved & 15))
        return fail(WUNET_E_ARG, "stoi loss: null argument (or tables / scratch / saved that are not 16-byte aligned)");
    const StoiShape& s = l.s;
    hipStream_t st = (hipStream_t)stream;
    char *sc = (char*)scratch, *sv = (char*)saved;
    StoiBuffers B{};
    B.nk = (int*)(sv + l.v_nk); B.kept = (int*)(sv + l.v_kept); B.inv = (int*)(sv + l.v_inv); B.pw = (float*)(sv + l.v_pw); B.reim = (float*)(sv + l.v_reim);
    B.energy = (double*)(sc + l.f_energy); B.res = (float*)(sc + l.f_res); B.part = (double*)(sc + l.f_part);
    double* score = (double*)(sc + l.f_score);
    if (const int rc = stoi_enqueue(clean, estimate, rows, row_len, s, tables, B, extended, st)) return rc;
    WUNET_LAUNCH(stoi_final_kernel, dim3((unsigned)rows), dim3(WUNET_THREADS), 0, st, (const double*)B.part, (const int*)(s.F0 > 0 ? B.nk : nullptr), s.nblk,
                 per_row_out, frames_out, score);
    WUNET_CHECK_LAUNCH();
    WUNET_LAUNCH(stoi_loss_final_kernel, dim3(1), dim3(WUNET_THREADS), 0, st, (const double*)score, (unsigned)rows, loss_out);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

int stoi_loss_backward(bool extended, const void* saved, const float* grad_loss, size_t rows, size_t row_len, int fs, const float* tables, void* scratch,
                       float* grad_estimate, void* stream)
{
    StoiLossShape l{};
    if (stoi_loss_shape(rows, row_len, fs, extended, l)) return WUNET_E_ARG;
    if (!saved || !grad_loss || !tables || !scratch || !grad_estimate || ((size_t)tables & 15) || ((size_t)scratch & 15) || ((size_t)saved & 15))
        return fail(WUNET_E_ARG, "stoi loss: null argument (or tables / scratch / saved that are not 16-byte aligned)");
    const StoiShape& s = l.s;
    hipStream_t st = (hipStream_t)stream;
    char* sc = (char*)scratch;
    const char* sv = (const char*)saved;
    const int* nk = (const int*)(sv + l.v_nk);
    float* fg = (float*)(sc + l.b_fg);
    float* g10k = s.L ? (float*)(sc + l.b_g10k) : grad_estimate;
    if (s.nblk > 0) {
        double* gr = (double*)(sc + l.b_gr);
        if (extended) {
            EstoiBwdArgs G{};
            G.pw = (const float*)(sv + l.v_pw); G.nk = nk; G.gl = grad_loss; G.M = s.M; G.Fmax = s.Fmax; G.nsmax = s.Fmax - WUNET_STOI_SEG + 1;
            G.inv_rows = 1.0 / (double)rows; G.blk = (double*)(sc + l.b_blk); G.gr = gr;
            const double blocks = 8.0 * rows * G.nsmax * WUNET_ESTOI_BLK;
            prof_begin(st, "estoi_segment_bwd_kernel", 0.0, 4.0 * 2.0 * s.M * WUNET_STOI_BP + blocks);
            WUNET_LAUNCH(estoi_segment_bwd_kernel, dim3((G.nsmax + WUNET_ESTOI_SGB - 1) / WUNET_ESTOI_SGB, (unsigned)rows), dim3(WUNET_THREADS), 0, st, G);
            prof_end(st);
            WUNET_CHECK_LAUNCH();
            prof_begin(st, "estoi_gather_kernel", 0.0, blocks + 4.0 * s.M * WUNET_STOI_BP + 8.0 * s.M * WUNET_STOI_BANDS);
            WUNET_LAUNCH(estoi_gather_kernel, dim3((s.Fmax * WUNET_STOI_BANDS + WUNET_THREADS - 1) / WUNET_THREADS, (unsigned)rows), dim3(WUNET_THREADS), 0, st, G);
            prof_end(st);
            WUNET_CHECK_LAUNCH();
        } else {
            StoiSegBwdArgs G{};
            G.pw = (const float*)(sv + l.v_pw); G.nk = nk; G.gl = grad_loss; G.M = s.M; G.Fmax = s.Fmax; G.clip = 1.0 + std::pow(10.0, 15.0 / 20.0);
            G.inv_rows = 1.0 / (double)rows; G.gr = gr;
            prof_begin(st, "stoi_segment_bwd_kernel", 0.0, 4.0 * 2.0 * s.M * WUNET_STOI_BP + 8.0 * s.M * WUNET_STOI_BANDS);
            WUNET_LAUNCH(stoi_segment_bwd_kernel, dim3((s.Fmax + WUNET_STOI_FB - 1) / WUNET_STOI_FB, (unsigned)rows), dim3(WUNET_THREADS), 0, st, G);
            prof_end(st);
            WUNET_CHECK_LAUNCH();
        }
        StoiSpecBwdArgs P{};
        P.reim = (const float*)(sv + l.v_reim); P.gr = gr; P.basis = tables; P.nk = nk; P.M = s.M; P.Fmax = s.Fmax; P.fg = fg;
        const unsigned mtiles = (s.M + WUNET_STFT_FM - 1) / WUNET_STFT_FM;
        prof_begin(st, "stoi_spec_bwd_kernel", 2.0 * s.M * WUNET_STOI_N * 2.0 * WUNET_STOI_BP, 4.0 * (2.0 * s.M * WUNET_STOI_BP + (double)s.M * WUNET_STOI_N));
        WUNET_LAUNCH(stoi_spec_bwd_kernel, dim3(2 * mtiles), dim3(WUNET_THREADS), 0, st, P);
        prof_end(st);
        WUNET_CHECK_LAUNCH();
    }
    {
        StoiUnframeArgs U{};
        U.fg = fg; U.w = tables + WUNET_STOI_TAB_W; U.inv = (const int*)(sv + l.v_inv); U.nk = s.nblk > 0 ? nk : nullptr; U.g = g10k;
        U.Tr = s.Tr; U.total = rows * s.Tr; U.Fmax = s.Fmax; U.F0 = s.F0;
        prof_begin(st, "stoi_unframe_kernel", 0.0, 4.0 * ((double)s.M * WUNET_STOI_N + rows * s.Tr));
        WUNET_LAUNCH(stoi_unframe_kernel, dim3((unsigned)((U.total + WUNET_THREADS - 1) / WUNET_THREADS)), dim3(WUNET_THREADS), 0, st, U);
        prof_end(st);
        WUNET_CHECK_LAUNCH();
    }
    if (s.L) {
        StoiResampleBwdArgs R{};
        R.gy = g10k; R.taps = tables + WUNET_STOI_TAB_TAPS; R.gx = grad_estimate; R.T = row_len; R.Tr = s.Tr; R.p = s.p; R.q = s.q; R.L = s.L;
        const unsigned per = WUNET_THREADS * WUNET_STOI_RPT;
        prof_begin(st, "stoi_resample_bwd_kernel", 2.0 * rows * row_len * ((2.0 * s.L + 1.0) / s.q), 4.0 * rows * (row_len + s.Tr));
        WUNET_LAUNCH(stoi_resample_bwd_kernel, dim3((unsigned)((row_len + per - 1) / per), (unsigned)rows), dim3(WUNET_THREADS), 0, st, R);
        prof_end(st);
        WUNET_CHECK_LAUNCH();
    }
    return WUNET_OK;
}
}  // namespace

int wunet_stoi_forward(const float* clean, const float* estimate, size_t rows, size_t row_len, int fs, const float* tables, void* scratch,
                       float* out, int* frames_out, void* stream)
{
    return stoi_forward(false, clean, estimate, rows, row_len, fs, tables, scratch, out, frames_out, stream);
}

size_t wunet_stoi_loss_scratch_bytes(size_t rows, size_t row_len, int fs) { return stoi_loss_bytes(false, false, rows, row_len, fs); }
size_t wunet_stoi_loss_saved_bytes(size_t rows, size_t row_len, int fs) { return stoi_loss_bytes(false, true, rows, row_len, fs); }

int wunet_stoi_loss_forward(const float* clean, const float* estimate, size_t rows, size_t row_len, int fs, const float* tables, void* scratch,
                            void* saved, float* loss_out, float* per_row_out, int* frames_out, void* stream)
{
    return stoi_loss_forward(false, clean, estimate, rows, row_len, fs, tables, scratch, saved, loss_out, per_row_out, frames_out, stream);
}

int wunet_stoi_loss_backward(const void* saved, const float* grad_loss, size_t rows, size_t row_len, int fs, const float* tables, void* scratch,
                             float* grad_estimate, void* stream)
{
    return stoi_loss_backward(false, saved, grad_loss, rows, row_len, fs, tables, scratch, grad_estimate, stream);
}

size_t wunet_estoi_scratch_bytes(size_t rows, size_t row_len, int fs) { return wunet_stoi_scratch_bytes(rows, row_len, fs); }

int wunet_estoi_forward(const float* clean, const float* estimate, size_t rows, size_t row_len, int fs, const float* tables, void* scratch,
                        float* out, int* frames_out, void* stream)
{
    return stoi_forward(true, clean, estimate, rows, row_len, fs, tables, scratch, out, frames_out, stream);
}

size_t wunet_estoi_loss_scratch_bytes(size_t rows, size_t row_len, int fs) { return stoi_loss_bytes(true, false, rows, row_len, fs); }
size_t wunet_estoi_loss_saved_bytes(size_t rows, size_t row_len, int fs) { return stoi_loss_bytes(true, true, rows, row_len, fs); }

int wunet_estoi_loss_forward(const float* clean, const float* estimate, size_t rows, size_t row_len, int fs, const float* tables, void* scratch,
                             void* saved, float* loss_out, float* per_row_out, int* frames_out, void* stream)
{
    return stoi_loss_forward(true, clean, estimate, rows, row_len, fs, tables, scratch, saved, loss_out, per_row_out, frames_out, stream);
}

int wunet_estoi_loss_backward(const void* saved, const float* grad_loss, size_t rows, size_t row_len, int fs, const float* tables, void* scratch,
                              float* grad_estimate, void* stream)
{
    return stoi_loss_backward(true, saved, grad_loss, rows, row_len, fs, tables, scratch, grad_estimate, stream);
}

// ---------------------------------------------------------------------------- fused Adam
// One launch of an Adam step: up to WUNET_ADAM_MAX tensors, grid (bx, cnt): blockIdx.y = tensor, blockIdx.x strides inside it.
struct AdamLaunch {
    AdamTable T;
    unsigned bx;
    int cnt;
};

static void adam_launch_at(int n_tensors, int base, float* const* params, const float* const* grads, float* const* exp_avg,
                           float* const* exp_avg_sq, const size_t* numels, AdamLaunch& L)
{
    L.T = AdamTable{};
    L.cnt = n_tensors - base < WUNET_ADAM_MAX ? n_tensors - base : WUNET_ADAM_MAX;
    size_t nmax = 0;
    for (int k = 0; k < L.cnt; ++k) {
        L.T.p[k] = params[base + k]; L.T.g[k] = grads[base + k]; L.T.m[k] = exp_avg[base + k]; L.T.v[k] = exp_avg_sq[base + k];
        L.T.n[k] = (unsigned)numels[base + k];
        if (numels[base + k] > nmax) nmax = numels[base + k];
    }
    L.bx = capped_blocks(nmax, WUNET_THREADS * 4, 256);
    if (L.bx < 1) L.bx = 1;
}

// What wunet_adam_step_ex has and wunet_adam_step has not.  on: the _ex entry - an 8-float hyper buffer, always filled by a hyper launch of
// one whole block; clip: the norm launches run, their partial sums in `scratch`.
struct AdamOptional {
    bool on = false, clip = false;
    double weight_decay = 0.0, max_grad_norm = 0.0;
    const double* lr_dev = nullptr;
    void* scratch = nullptr;
};

// The launches of one step, in order: the norm's (they write their partial sums one behind the other), the hyper launch, the updates.
// The plain entry without a device counter has no hyper launch: its two scalars come from the host's pow and travel as kernel
// arguments.  With one it launches ONE thread (no partial sums: no barrier) and the kernels stay inside its 2-float buffer.
static int adam_enqueue(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                        const size_t* numels, double lr, double beta1, double beta2, double eps, long long step, double grad_scale,
                        long long* step_dev, float* hyper_dev, const AdamOptional& O, hipStream_t st)
{
    AdamLaunch L;
    int n_part = 0;
    for (int base = 0; O.clip && base < n_tensors; base += WUNET_ADAM_MAX) {
        adam_launch_at(n_tensors, base, params, grads, exp_avg, exp_avg_sq, numels, L);
        WUNET_LAUNCH(grad_sqnorm_partial_kernel, dim3(L.bx, L.cnt), dim3(WUNET_THREADS), 0, st, L.T, (float)grad_scale, (double*)O.scratch + n_part);
        WUNET_CHECK_LAUNCH();
        n_part += (int)L.bx * L.cnt;
    }
    const bool on_device = O.on || step_dev;          // who computes step_size and bc2_sqrt
    float step_size = 0.0f, bc2_sqrt = 1.0f;
    if (on_device) {
        WUNET_LAUNCH(adam_hyper_kernel, dim3(1), dim3(O.on ? WUNET_THREADS : 1), 0, st, step_dev, step, lr, O.lr_dev, beta1, beta2, O.weight_decay,
                     O.max_grad_norm, (const double*)O.scratch, n_part, hyper_dev, O.on);
        WUNET_CHECK_LAUNCH();
    } else {
        const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
        step_size = (float)(lr / bc1); bc2_sqrt = (float)sqrt(bc2);
    }
    for (int base = 0; base < n_tensors; base += WUNET_ADAM_MAX) {
        adam_launch_at(n_tensors, base, params, grads, exp_avg, exp_avg_sq, numels, L);
        WUNET_LAUNCH(adam_kernel, dim3(L.bx, L.cnt), dim3(WUNET_THREADS), 0, st, L.T, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                     bc2_sqrt, (float)eps, step_size, (float)grad_scale, (const float*)(on_device ? hyper_dev : nullptr), O.on);
        WUNET_CHECK_LAUNCH();
    }
    return WUNET_OK;
}

int wunet_adam_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                    float* const* exp_avg_sq, const size_t* numels, double lr, double beta1, double beta2, double eps,
                    long long step, double grad_scale, long long* step_dev, float* hyper_dev, void* stream)
{
    if (n_tensors < 0 || (n_tensors > 0 && (!params || !grads || !exp_avg || !exp_avg_sq || !numels))) return fail(WUNET_E_ARG, "null argument");
    if (!step_dev && step < 1) return fail(WUNET_E_ARG, "step must be >= 1");
    if (step_dev && !hyper_dev) return fail(WUNET_E_ARG, "a device step counter needs the 2-float hyper buffer");
    for (int k = 0; k < n_tensors; ++k)          // (before anything is enqueued: a refused call leaves the device counter alone)
        if (numels[k] >= (1ull << 32)) return fail(WUNET_E_ARG, "tensor too large");
    return adam_enqueue(n_tensors, params, grads, exp_avg, exp_avg_sq, numels, lr, beta1, beta2, eps, step, grad_scale, step_dev, hyper_dev,
                        AdamOptional{}, (hipStream_t)stream);
}

// one double per block of the norm's launches: at most 256 blocks per tensor
size_t wunet_adam_scratch_bytes(int n_tensors) { return n_tensors > 0 ? (size_t)n_tensors * 256 * sizeof(double) : 0; }

int wunet_adam_step_ex(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                       float* const* exp_avg_sq, const size_t* numels, double lr, double beta1, double beta2, double eps,
                       long long step, double grad_scale, double weight_decay, double max_grad_norm, long long* step_dev,
                       float* hyper_dev, const double* lr_dev, void* scratch, void* stream)
{
    if (n_tensors < 0 || (n_tensors > 0 && (!params || !grads || !exp_avg || !exp_avg_sq || !numels))) return fail(WUNET_E_ARG, "null argument");
    if (!hyper_dev) return fail(WUNET_E_ARG, "wunet_adam_step_ex needs the hyper buffer (WUNET_ADAM_HYPER_FLOATS floats)");
    if (!step_dev && step < 1) return fail(WUNET_E_ARG, "step must be >= 1");
    if (!(weight_decay >= 0.0)) return fail(WUNET_E_ARG, "weight_decay must be >= 0 (got %g)", weight_decay);
    if (max_grad_norm != max_grad_norm) return fail(WUNET_E_ARG, "max_grad_norm is NaN");
    const bool clip = max_grad_norm > 0.0 && n_tensors > 0;
    if (clip && !scratch) return fail(WUNET_E_ARG, "max_grad_norm > 0 needs wunet_adam_scratch_bytes(n_tensors) bytes of scratch");
    for (int k = 0; k < n_tensors; ++k)          // (before anything is enqueued: a refused call leaves the device counter alone)
        if (numels[k] >= (1ull << 32)) return fail(WUNET_E_ARG, "tensor too large");
    return adam_enqueue(n_tensors, params, grads, exp_avg, exp_avg_sq, numels, lr, beta1, beta2, eps, step, grad_scale, step_dev, hyper_dev,
                        AdamOptional{true, clip, weight_decay, max_grad_norm, lr_dev, scratch}, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------- profiler
int wunet_profile_enable(int on)
{
    g_prof_on = on != 0;
    return WUNET_OK;
}

// Writes one line per kernel name: "name\tlaunches\ttotal_ms\ttotal_flops\ttotal_bytes\n"; clears the records.
// Synchronises the device.  Returns the number of bytes written (<= cap-1) or a negative code.
long long wunet_profile_collect(char* buf, size_t cap) { return prof_collect(buf, cap); }

void wunet_debug_set_conv_trace(void* dev_buffer) { g_h3_trace = static_cast<unsigned long long*>(dev_buffer); }

// ---------------------------------------------------------------------------- data input
// Aligned crops of the (mixture, clean) pair out of two flat float32 arrays resident in HBM: window b is samples
// starts[b] .. starts[b] + length - 1 of both arrays - the reference's per-item crop (util/utils.py:101-113,
// dataset/waveform_dataset.py:56-67) for a whole batch in one launch.  The window starts are device-side int64 (drawn on the
// host, uploaded with the batch's other 8 B x batch of metadata); out rows are [batch][1][length].
int wunet_crop_windows(const float* mixture_flat, const float* clean_flat, const long long* starts, long long total,
                       int batch, int length, float* mixture, float* clean, void* stream)
{
    if (!mixture_flat || !clean_flat || !starts || !mixture || !clean) return fail(WUNET_E_ARG, "null argument");
    if (batch < 1 || length < 1 || total < length) return fail(WUNET_E_ARG, "bad crop shape (batch=%d length=%d total=%lld)", batch, length, total);
    hipStream_t st = (hipStream_t)stream;
    const unsigned bx = (unsigned)((length + 4 * WUNET_THREADS - 1) / (4 * WUNET_THREADS));
    WUNET_LAUNCH(crop_windows_kernel, dim3(bx, (unsigned)batch), dim3(WUNET_THREADS), 0, st, mixture_flat, clean_flat, starts, total, length,
                 mixture, clean);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

// ---------------------------------------------------------------------------- data input: mixtures made on the device (wunet_mix.h)
#define WUNET_MIX_BLOCKS 1024
#define WUNET_MIX_MIN_PIECE 1024         // one trip of 4 samples per thread

// ---- the checks that the row-table ops share.  n windows of `length` samples: the rows are a grid's y (the loader ops' batch), with
// `chunks` its x (the chunk ops' n).  `op` starts the messages; nullptr: a size query, which answers 0 without a message.
static int window_shape_check(const char* op, long long n, int length, bool chunks)
{
    if (n >= 1 && length >= 1 && n <= (chunks ? 0x7fffffffLL : 65535LL) && length <= (1 << 30)) return 0;
    if (!op) return WUNET_E_ARG;
    if (n < 1 || length < 1) return fail(WUNET_E_ARG, "%s: %s and length must be >= 1 (got %lld x %d)", op, chunks ? "n" : "batch", n, length);
    return fail(WUNET_E_ARG, "%s: at most %s of 2^30 samples per call (got %lld x %d)", op, chunks ? "2^31 - 1 chunks" : "65535 rows", n, length);
}
// a flat array's total (or its longest row) in [lo, limit); rows of a multiple of 4 samples move 16 bytes at a time: a, b (or null) aligned so
static bool total_in_range(long long total, long long lo, long long limit) { return total >= lo && total < limit; }
static bool rows_misaligned(int length, const void* a, const void* b) { return (length & 3) == 0 && (((size_t)a | (size_t)b) & 15); }

size_t wunet_mix_scratch_bytes(int batch, int length)
{
    if (window_shape_check(nullptr, batch, length, false)) return 0;
    size_t ppr, plen;
    row_pieces((size_t)batch, (size_t)length, WUNET_MIX_BLOCKS, WUNET_MIX_MIN_PIECE, ppr, plen);
    return (size_t)batch * ppr * WUNET_MIX_PART * sizeof(double);
}

int wunet_mix_windows(const float* clean_flat, long long clean_total, const float* noise_flat, long long noise_total, const long long* rows,
                      const float* params, float peak_limit, int batch, int length, void* scratch, float* mixture, float* clean_out,
                      float* gains, void* stream)
{
    if (window_shape_check("mix", batch, length, false)) return WUNET_E_ARG;
    if (clean_total < length) return fail(WUNET_E_ARG, "mix: the clean array is shorter than one window (clean_total=%lld length=%d)", clean_total, length);
    if (noise_total < 1) return fail(WUNET_E_ARG, "mix: the noise array is empty (noise_total=%lld)", noise_total);
    if (clean_total >= (1LL << 60) || noise_total >= (1LL << 60)) return fail(WUNET_E_ARG, "mix: array too large");
    if (!clean_flat || !noise_flat || !rows || !params || !scratch || !mixture || !clean_out) return fail(WUNET_E_ARG, "mix: null argument");
    if (!(peak_limit == peak_limit)) return fail(WUNET_E_ARG, "mix: peak_limit is NaN");
    if (((size_t)scratch & 7) || rows_misaligned(length, mixture, clean_out))
        return fail(WUNET_E_ARG, "mix: scratch needs 8-byte alignment, the outputs 16-byte alignment when length %% 4 == 0");
    hipStream_t st = (hipStream_t)stream;
    MixArgs A{};
    A.clean_flat = clean_flat; A.noise_flat = noise_flat; A.clean_total = clean_total; A.noise_total = noise_total; A.rows = rows;
    A.params = params; A.peak_limit = peak_limit; A.length = length; A.part = (double*)scratch; A.mixture = mixture; A.clean_out = clean_out;
    A.gains = gains;
    size_t ppr, plen;
    row_pieces((size_t)batch, (size_t)length, WUNET_MIX_BLOCKS, WUNET_MIX_MIN_PIECE, ppr, plen);
    A.ppr = (unsigned)ppr; A.plen = (int)plen;
    const double n = (double)batch * length;
    prof_begin(st, "mix_partial_kernel", 4.0 * n, 4.0 * 2.0 * n);
    WUNET_LAUNCH(mix_partial_kernel, dim3((unsigned)batch * A.ppr), dim3(WUNET_THREADS), 0, st, A);
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    prof_begin(st, "mix_apply_kernel", 3.0 * n, 4.0 * 4.0 * n);
    WUNET_LAUNCH(mix_apply_kernel, dim3(A.ppr, (unsigned)batch), dim3(WUNET_THREADS), 0, st, A);
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

// dst = a src with the a that wunet_mix_windows wrote into `gains` (a target that is not the window the mix read, at the mixture's level)
int wunet_apply_level(const float* src, const float* gains, int batch, int length, float* dst, void* stream)
{
    if (window_shape_check("mix", batch, length, false)) return WUNET_E_ARG;
    if (!src || !gains || !dst) return fail(WUNET_E_ARG, "apply_level: null argument");
    if (rows_misaligned(length, src, dst)) return fail(WUNET_E_ARG, "apply_level: src and dst need 16-byte alignment when length %% 4 == 0");
    hipStream_t st = (hipStream_t)stream;
    const double n = (double)batch * length;
    prof_begin(st, "apply_level_kernel", n, 4.0 * 2.0 * n);
    WUNET_LAUNCH(apply_level_kernel, dim3((unsigned)((length + 4 * WUNET_THREADS - 1) / (4 * WUNET_THREADS)), (unsigned)batch), dim3(WUNET_THREADS), 0, st,
                 src, gains, length, dst);
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

// ---------------------------------------------------------------------------- data input: reverberant speech (wunet_reverb.h)
int wunet_reverb_windows(const float* clean_flat, long long clean_total, const float* rir_flat, long long rir_total, const long long* rows,
                         int early_taps, int batch, int length, float* reverberant, float* direct, void* stream)
{
    if (window_shape_check("reverb", batch, length, false)) return WUNET_E_ARG;
    if (clean_total < length) return fail(WUNET_E_ARG, "reverb: the clean array is shorter than one window (clean_total=%lld length=%d)", clean_total, length);
    if (rir_total < 1) return fail(WUNET_E_ARG, "reverb: the rir array is empty (rir_total=%lld)", rir_total);
    if (clean_total >= (1LL << 60) || rir_total >= (1LL << 60)) return fail(WUNET_E_ARG, "reverb: array too large");
    if (!clean_flat || !rir_flat || !rows || !reverberant) return fail(WUNET_E_ARG, "reverb: null argument");
    if (direct && early_taps < 1) return fail(WUNET_E_ARG, "reverb: early_taps must be >= 1 when direct is given (got %d)", early_taps);
    if (rows_misaligned(length, reverberant, direct))
        return fail(WUNET_E_ARG, "reverb: the outputs need 16-byte alignment when length %% 4 == 0");
    hipStream_t st = (hipStream_t)stream;
    ReverbArgs A{};
    A.clean_flat = clean_flat; A.rir_flat = rir_flat; A.clean_total = clean_total; A.rir_total = rir_total; A.rows = rows;
    A.early_taps = early_taps; A.length = length; A.reverberant = reverberant; A.direct = direct;
    const double n = (double)batch * length;
    // (the taps are the tables': the profiler's FLOP column counts one tap per sample, the bytes the two outputs)
    prof_begin(st, "reverb_kernel", 2.0 * n, 4.0 * 3.0 * n);
    WUNET_LAUNCH(reverb_kernel, dim3((unsigned)((length + WUNET_REVERB_CH - 1) / WUNET_REVERB_CH), (unsigned)batch), dim3(WUNET_THREADS), 0, st, A);
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

// ---------------------------------------------------------------------------- chunked enhancement with overlap (wunet_chunks.h)
static unsigned chunk_pieces_y(long long pieces) { return (unsigned)(pieces < (long long)WUNET_CHUNK_MAX_Y ? pieces : (long long)WUNET_CHUNK_MAX_Y); }

int wunet_chunk_gather(const float* flat, long long total, const long long* rows, long long n, int length, float* chunks, void* stream)
{
    if (window_shape_check("chunk_gather", n, length, true)) return WUNET_E_ARG;
    if (!total_in_range(total, 1, WUNET_CHUNK_LIMIT)) return fail(WUNET_E_ARG, "chunk_gather: bad size of the flat array (total=%lld)", total);
    if (!flat || !rows || !chunks) return fail(WUNET_E_ARG, "chunk_gather: null argument");
    hipStream_t st = (hipStream_t)stream;
    const long long pieces = ((long long)length + WUNET_CHUNK_PIECE - 1) / WUNET_CHUNK_PIECE;
    const double cnt = (double)n * length;
    prof_begin(st, "chunk_gather_kernel", 0.0, 4.0 * 2.0 * cnt);
    WUNET_LAUNCH(chunk_gather_kernel, dim3((unsigned)n, chunk_pieces_y(pieces)), dim3(WUNET_THREADS), 0, st, flat, total, rows, length, chunks);
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

int wunet_chunk_overlap_add(const float* chunks, long long n, int length, int margin, int fade, const float* ramp, const long long* recs,
                            long long n_recs, long long max_len, float* out_flat, long long total, void* stream)
{
    if (window_shape_check("chunk_overlap_add", n, length, true)) return WUNET_E_ARG;
    if (margin < 0 || fade < 0) return fail(WUNET_E_ARG, "chunk_overlap_add: margin and fade must be >= 0 (got %d, %d)", margin, fade);
    const long long hop = (long long)length - 2LL * margin - fade;
    if (hop < 1 || fade > hop)
        return fail(WUNET_E_ARG, "chunk_overlap_add: the hop length - 2 margin - fade must be >= 1 and >= fade (length=%d margin=%d fade=%d)", length, margin, fade);
    if ((fade > 0) != (ramp != nullptr)) return fail(WUNET_E_ARG, "chunk_overlap_add: ramp must be given exactly when fade > 0 (fade=%d)", fade);
    if (n_recs < 1 || n_recs > 0x7fffffffLL) return fail(WUNET_E_ARG, "chunk_overlap_add: n_recs must be in [1, 2^31) (got %lld)", n_recs);
    if (!total_in_range(max_len, 1, WUNET_CHUNK_LIMIT)) return fail(WUNET_E_ARG, "chunk_overlap_add: bad max_len (%lld)", max_len);
    if (!total_in_range(total, 1, WUNET_CHUNK_LIMIT)) return fail(WUNET_E_ARG, "chunk_overlap_add: bad size of the flat output (total=%lld)", total);
    if (!chunks || !recs || !out_flat) return fail(WUNET_E_ARG, "chunk_overlap_add: null argument");
    hipStream_t st = (hipStream_t)stream;
    ChunkOlaArgs A{};
    A.chunks = chunks; A.n = n; A.length = length; A.margin = margin; A.fade = fade; A.hop = (int)hop; A.ramp = ramp; A.recs = recs;
    A.pieces = (max_len + WUNET_CHUNK_PIECE - 1) / WUNET_CHUNK_PIECE; A.out_flat = out_flat; A.total = total;
    prof_begin(st, "chunk_overlap_add_kernel", 0.0, 4.0 * 2.0 * (double)total);
    WUNET_LAUNCH(chunk_overlap_add_kernel, dim3((unsigned)n_recs, chunk_pieces_y(A.pieces)), dim3(WUNET_THREADS), 0, st, A);
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

// ---------------------------------------------------------------------------- rational resampling of ragged rows (wunet_resample.h)
static long long gcd_ll(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; }

// the argument checks shared by the two entries: 0, or -1 with the message set
static int resample_filter_check(int up, int down, int n_taps)
{
    if (up < 1 || down < 1) return fail(WUNET_E_ARG, "resample: up and down must be >= 1 (got %d / %d)", up, down);
    if (gcd_ll(up, down) != 1) return fail(WUNET_E_ARG, "resample: up / down must be in lowest terms, coprime (got %d / %d)", up, down);
    if (up > WUNET_RESAMPLE_MAX_RATIO || down > WUNET_RESAMPLE_MAX_RATIO)
        return fail(WUNET_E_ARG, "resample: max(up, down) is above the cap of %d (got %d / %d)", WUNET_RESAMPLE_MAX_RATIO, up, down);
    if (n_taps < 1 || (n_taps & 1) == 0) return fail(WUNET_E_ARG, "resample: n_taps = 2 L + 1 must be odd (got %d)", n_taps);
    if (n_taps > WUNET_RESAMPLE_MAX_TAPS) return fail(WUNET_E_ARG, "resample: n_taps is above the cap of %d taps (got %d)", WUNET_RESAMPLE_MAX_TAPS, n_taps);
    return 0;
}

long long wunet_resample_tile(int up, int down, int n_taps)
{
    if (resample_filter_check(up, down, n_taps)) return 0;
    return wunet_lds::resample(up, down, n_taps).tile;
}

int wunet_resample_rows(const float* in, long long in_total, const long long* rows, long long n, long long max_out, int up, int down,
                        const float* taps, int n_taps, float* out, long long out_total, void* stream)
{
    if (n < 1 || max_out < 1) return fail(WUNET_E_ARG, "resample: n and max_out must be >= 1 (got %lld, %lld)", n, max_out);
    if (n > 0x7fffffffLL) return fail(WUNET_E_ARG, "resample: at most 2^31 - 1 rows per call (got %lld)", n);
    if (resample_filter_check(up, down, n_taps)) return WUNET_E_ARG;
    if (!total_in_range(in_total, 1, WUNET_RESAMPLE_LIMIT) || !total_in_range(out_total, 1, WUNET_RESAMPLE_LIMIT))
        return fail(WUNET_E_ARG, "resample: bad size of an array (in_total=%lld out_total=%lld)", in_total, out_total);
    if (!in || !rows || !taps || !out) return fail(WUNET_E_ARG, "resample: null argument");
    hipStream_t st = (hipStream_t)stream;
    const wunet_lds::Resample lay = wunet_lds::resample(up, down, n_taps);
    if (max_out > out_total) max_out = out_total;
    ResampleArgs A{};
    A.in = in; A.in_total = in_total; A.rows = rows; A.max_out = max_out; A.tiles = (max_out + lay.tile - 1) / lay.tile;
    A.up = up; A.down = down; A.half = (n_taps - 1) / 2; A.taps = taps;
    A.g = lay.g; A.ng = lay.ng; A.tile = lay.tile; A.span = lay.span; A.ntaps = n_taps; A.out = out; A.out_total = out_total;
    long long y = (WUNET_RESAMPLE_BLOCKS + n - 1) / n;
    if (y > A.tiles) y = A.tiles;
    if (y > (long long)WUNET_CHUNK_MAX_Y) y = WUNET_CHUNK_MAX_Y;
    if (WUNET_ALLOW_BIG_LDS(resample_rows_kernel, lay.bytes())) return fail(WUNET_E_RUNTIME, "resample: %zu bytes of LDS were not granted", lay.bytes());
    // (the profiler's columns for rows of max_out outputs: the terms of an output, the samples in and out)
    const double outs = (double)n * (double)max_out;
    prof_begin(st, "resample_rows_kernel", 2.0 * outs * ((n_taps - 1) / up + 1), 4.0 * outs * (1.0 + (double)down / up));
    WUNET_LAUNCH(resample_rows_kernel, dim3((unsigned)n, (unsigned)y), dim3(WUNET_THREADS), lay.bytes(), st, A);
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

// ---------------------------------------------------------------------------- cascades of second-order sections (wunet_sos.h)
static int sos_sections_check(int sections)
{
    if (sections >= 1 && sections <= WUNET_SOS_MAX_SECTIONS) return 0;
    return fail(WUNET_E_ARG, "sos: sections must be in [1, %d] (got %d)", WUNET_SOS_MAX_SECTIONS, sections);
}

long long wunet_sos_tile(int sections)
{
    if (sos_sections_check(sections)) return 0;
    return ((long long)wunet_lds::kSosTile << 16) | (long long)wunet_lds::kSosChunk;
}

extern "C++" template <int S>
int sos_launch(const SosArgs& A, int batch, hipStream_t st)
{
    constexpr size_t bytes = wunet_lds::sos(S).bytes();
    if (WUNET_ALLOW_BIG_LDS(sos_windows_kernel<S>, bytes)) return fail(WUNET_E_RUNTIME, "sos: %zu bytes of LDS were not granted", bytes);
    const double n = (double)batch * ((double)A.lead + A.length);
    // (the profiler's columns: two passes of 9 flops per sample and section; the samples in and out)
    prof_begin(st, "sos_windows_kernel", 2.0 * 9.0 * S * n, 4.0 * 2.0 * n);
    WUNET_LAUNCH(sos_windows_kernel<S>, dim3((unsigned)batch), dim3(WUNET_THREADS), bytes, st, A);
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

int wunet_sos_windows(const float* flat, long long total, const long long* rows, const float* coefs, int sections, int lead, int batch,
                      int length, float* out, void* stream)
{
    if (batch < 1 || length < 1) return fail(WUNET_E_ARG, "sos: batch and length must be >= 1 (got %d x %d)", batch, length);
    if (batch > 65535 || length > (1 << 24)) return fail(WUNET_E_ARG, "sos: at most 65535 rows of 2^24 samples per call (got %d x %d)", batch, length);
    if (sos_sections_check(sections)) return WUNET_E_ARG;
    if (lead < 0 || lead > WUNET_SOS_MAX_LEAD) return fail(WUNET_E_ARG, "sos: lead must be in [0, %d] (got %d)", WUNET_SOS_MAX_LEAD, lead);
    if (total < length) return fail(WUNET_E_ARG, "sos: the flat array is shorter than one window (total=%lld length=%d)", total, length);
    if (total >= (1LL << 60)) return fail(WUNET_E_ARG, "sos: array too large");
    if (!flat || !rows || !coefs || !out) return fail(WUNET_E_ARG, "sos: null argument");
    hipStream_t st = (hipStream_t)stream;
    SosArgs A{};
    A.flat = flat; A.total = total; A.rows = rows; A.coefs = coefs; A.lead = lead; A.length = length; A.out = out;
    switch (sections) {
    case 1: return sos_launch<1>(A, batch, st);
    case 2: return sos_launch<2>(A, batch, st);
    case 3: return sos_launch<3>(A, batch, st);
    case 4: return sos_launch<4>(A, batch, st);
    case 5: return sos_launch<5>(A, batch, st);
    case 6: return sos_launch<6>(A, batch, st);
    case 7: return sos_launch<7>(A, batch, st);
    default: return sos_launch<8>(A, batch, st);
    }
}

// ---------------------------------------------------------------------------- BSS Eval SDR per row (wunet_bss.h)
static int bss_check(size_t rows, size_t row_len, int filter_length)
{
    if (filter_length < 1 || filter_length > WUNET_BSS_MAX_FILTER)
        return fail(WUNET_E_ARG, "bss_sdr: filter_length must be in [1, %d] (got %d)", WUNET_BSS_MAX_FILTER, filter_length);
    if (rows == 0 || row_len == 0) return fail(WUNET_E_ARG, "bss_sdr: rows and row_len must be > 0 (got %zu x %zu)", rows, row_len);
    if (rows > 65535 || row_len >= (1ull << 31))
        return fail(WUNET_E_ARG, "bss_sdr: at most 65535 rows of fewer than 2^31 samples per call (got %zu x %zu)", rows, row_len);
    return 0;
}

static unsigned bss_segments(size_t row_len) { return (unsigned)((row_len + wunet_lds::kBssTile - 1) / wunet_lds::kBssTile); }

long long wunet_bss_sdr_tile(int filter_length)
{
    if (bss_check(1, 1, filter_length)) return 0;
    return wunet_lds::kBssTile;
}

size_t wunet_bss_sdr_scratch_bytes(size_t rows, size_t row_len, int filter_length)
{
    if (bss_check(rows, row_len, filter_length)) return 0;
    return rows * bss_segments(row_len) * (size_t)(2 * filter_length + 1) * sizeof(double);
}

int wunet_bss_sdr_forward(const float* clean, const float* estimate, size_t rows, size_t row_len, const long long* lengths, int filter_length,
                          void* scratch, float* out_db, void* stream)
{
    if (bss_check(rows, row_len, filter_length)) return WUNET_E_ARG;
    if (!clean || !estimate || !scratch || !out_db) return fail(WUNET_E_ARG, "bss_sdr: null argument");
    hipStream_t st = (hipStream_t)stream;
    BssArgs A{};
    A.clean = clean; A.est = estimate; A.row_len = row_len; A.lengths = lengths; A.n = filter_length; A.segs = bss_segments(row_len);
    A.part = (double*)scratch; A.out = out_db;
    const double samples = (double)rows * (double)row_len;
    // (the profiler's columns: two products per lag and sample; both rows in, one partial per segment out)
    prof_begin(st, "bss_corr_kernel", 2.0 * 2.0 * filter_length * samples, 4.0 * 2.0 * samples);
    WUNET_LAUNCH(bss_corr_kernel, dim3(A.segs, (unsigned)rows), dim3(WUNET_THREADS), wunet_lds::bss_corr(filter_length).bytes(), st, A);
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    prof_begin(st, "bss_solve_kernel", (double)rows * 6.0 * filter_length * filter_length, 8.0 * (double)rows * A.segs * (2.0 * filter_length + 1.0));
    WUNET_LAUNCH(bss_solve_kernel, dim3((unsigned)rows), dim3(WUNET_THREADS), wunet_lds::bss_solve().bytes(), st, A);
    prof_end(st);
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

// ---------------------------------------------------------------------------- single-op entry points
static int op_check(int B, int Cin, int Cout, int L, int K)
{
    if (K != 5 && K != 15) return fail(WUNET_E_ARG, "K must be 5 or 15");
    if (B < 1 || Cin < 1 || Cout < 1 || !is_pow2(L) || L < 4) return fail(WUNET_E_ARG, "bad op shape (L must be a power of two >= 4)");
    return 0;
}

static int op_conv_common(const float* x, const float* w, const float* bias, float* out, int B, int kch, int rows,
                          int Cout, int Cin, int L, int K, int transposed, hipStream_t st)
{
    const ConvCfg cfg = plan_conv(B, L, rows, kch, K);
    float *wpk = nullptr, *part = nullptr;
    if (hipMalloc((void**)&wpk, (size_t)cfg.mtiles_p * cfg.cp * K * 16 * sizeof(float)) != hipSuccess) return fail(WUNET_E_RUNTIME, "hipMalloc");
    const size_t nout = (size_t)B * rows * L;
    if (cfg.ksplit > 1 && hipMalloc((void**)&part, (size_t)cfg.ksplit * nout * sizeof(float)) != hipSuccess) return fail(WUNET_E_RUNTIME, "hipMalloc");
    PackTable tab{};
    PackDesc& d = tab.d[0];
    d.w = w; d.dst = wpk; d.Cout = Cout; d.Cin = Cin; d.taps = K; d.M = rows; d.CP = cfg.cp; d.mtiles = cfg.mtiles_p; d.transposed = transposed;
    WUNET_LAUNCH(pack_weights_kernel, dim3(64, 1), dim3(WUNET_THREADS), 0, st, tab);
    const bool split = cfg.ksplit > 1;
    const ConvArgs a = make_conv_args(x, kch, wpk, split ? nullptr : bias, split ? part : out, nullptr, B, rows, L, K, cfg, nout);
    int rc = launch_conv(K, a, cfg, st);
    if (!rc && split) {
        WUNET_LAUNCH(split_sum_kernel, dim3(capped_blocks(nout, WUNET_THREADS, 2048)), dim3(WUNET_THREADS), 0, st, (const float*)part, cfg.ksplit, nout, out,
                     bias, rows, ilog2(L));
    }
    hipStreamSynchronize(st);
    hipFree(wpk);
    if (part) hipFree(part);
    if (rc) return rc;
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

int wunet_op_conv1d(const float* x, const float* w, const float* bias, float* z, int B, int Cin, int Cout, int L, int K, void* stream)
{
    if (op_check(B, Cin, Cout, L, K)) return WUNET_E_ARG;
    return op_conv_common(x, w, bias, z, B, Cin, Cout, Cout, Cin, L, K, 0, (hipStream_t)stream);
}

int wunet_op_conv1d_dgrad(const float* gz, const float* w, float* dx, int B, int Cin, int Cout, int L, int K, void* stream)
{
    if (op_check(B, Cin, Cout, L, K)) return WUNET_E_ARG;
    return op_conv_common(gz, w, nullptr, dx, B, Cout, Cin, Cout, Cin, L, K, 1, (hipStream_t)stream);
}

int wunet_op_conv1d_wgrad(const float* gz, const float* x, float* dw, int B, int Cin, int Cout, int L, int K, void* stream)
{
    if (op_check(B, Cin, Cout, L, K)) return WUNET_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const WgradCfg cfg = plan_wgrad(B, L, Cin, Cout, K);
    float* part = nullptr;
    const size_t nw = (size_t)Cout * Cin * K;
    if (hipMalloc((void**)&part, (size_t)cfg.rows * nw * sizeof(float)) != hipSuccess) return fail(WUNET_E_RUNTIME, "hipMalloc");
    const WgradArgs a = make_wgrad_args(x, gz, part, B, Cin, Cout, L, K, cfg.cps);
    int rc = launch_wgrad_any(K, a, cfg, st);
    if (!rc) {
        WUNET_LAUNCH(wgrad_reduce_kernel, dim3(capped_blocks(nw, WUNET_THREADS, 2048)), dim3(WUNET_THREADS), 0, st, (const float*)part, cfg.rows, nw, dw);
    }
    hipStreamSynchronize(st);
    hipFree(part);
    if (rc) return rc;
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

// ---- single-op entry points of the fp16-split kernels: the same planner, operand passes and GEMM kernels the network
//      uses for that geometry (scales from the measured maxima, as in eval mode).  bf: their bf16 mode (wunet_set_h3(ctx, 3 | 4):
//      one bf16 word per operand value in the hi plane, the lo plane unused, one MFMA pass), the wunet_op_*_bf16 entry points
namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;            // (a kernel-launch lambda must capture the raw pointer, never the owner)
    bool alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16) == hipSuccess; }
    float* f() const { return (float*)p; }
    wunet_half* h() const { return (wunet_half*)p; }
};

int op_split_check(int B, int Cin, int Cout, int L, int K, bool backward)
{
    if (op_check(B, Cin, Cout, L, K)) return WUNET_E_ARG;
    if (L < 16 || (long long)B * L < 256) return fail(WUNET_E_ARG, "the split kernels need L >= 16 and B*L >= 256");
    if (backward && Cin < 16) return fail(WUNET_E_ARG, "the split data / weight gradient needs Cin >= 16");
    return 0;
}

// fp32 [B][C][L] -> scaled hi / lo in the split layout; slot: 8 floats, [0..1] receive {scale, 1/scale}, [4] the measured max
// (one allocation: hi plane | lo plane | 64 zero bytes - the layout conv_h3d_kernel's DMA addressing wants, launch_conv_h3; the
// bf16 mode writes the hi plane only)
struct SplitBuf {
    DevBuf buf;
    size_t plane = 0;
    wunet_half* h() const { return buf.h(); }
    wunet_half* l() const { return reinterpret_cast<wunet_half*>(static_cast<char*>(buf.p) + plane); }
    const void* zpad() const { return static_cast<char*>(buf.p) + 2 * plane; }
};
int op_split_operand(const float* x, int B, int C, int L, SplitBuf& sb, float* slot, const float* ones, const float* zeros, int bf, hipStream_t st)
{
    const int c8 = (C + 7) / 8;
    sb.plane = (size_t)B * c8 * L * 16;
    if (!sb.buf.alloc(2 * sb.plane + 64)) return fail(WUNET_E_RUNTIME, "hipMalloc");
    hipMemsetAsync(static_cast<char*>(sb.buf.p) + 2 * sb.plane, 0, 64, st);
    hipMemsetAsync(slot, 0, WUNET_SLOT_FLOATS * sizeof(float), st);
    const size_t n4 = (size_t)B * C * L / 4;
    WUNET_LAUNCH(act_max_kernel, dim3(capped_blocks(n4, WUNET_THREADS * 4, 2048)), dim3(WUNET_THREADS), 0, st, x, ones, zeros, C, ilog2(L), n4, slot + 4);
    return launch_split(x, sb.h(), sb.l(), nullptr, slot + 4, nullptr, slot, B, C, L, st, bf);
}

int op_conv_split_common(const float* x, const float* w, const float* bias, float* out, int B, int kch, int rows, int Cout, int Cin,
                         int L, int K, int transposed, int bf, hipStream_t st)
{
    const H3ConvPlan p = plan_h3_conv(B, L, rows, kch, K, transposed != 0, bf, read_plan_switches());
    SplitBuf xs;
    DevBuf wpk, misc, part;
    const size_t wh_halfs = (size_t)p.mtp * p.nch * K * 512, nout = (size_t)B * rows * L;
    // misc: slot of x (8 floats) | slot of w (8) | partial weight maxima | ones (kch) | zeros (kch)
    if (!wpk.alloc(wh_halfs * 4) || !misc.alloc((16 + WUNET_WMAX_PARTS + 2 * (size_t)kch) * sizeof(float)) ||
        (p.ksplit > 1 && !part.alloc((size_t)p.ksplit * nout * sizeof(float))))
        return fail(WUNET_E_RUNTIME, "hipMalloc");
    float* xslot = misc.f(), *wslot = misc.f() + 8, *wmax = misc.f() + 16, *oz = misc.f() + 16 + WUNET_WMAX_PARTS;
    WUNET_LAUNCH(fill_kernel, dim3(4), dim3(WUNET_THREADS), 0, st, oz, (size_t)kch, 1.0f);
    WUNET_LAUNCH(fill_kernel, dim3(4), dim3(WUNET_THREADS), 0, st, oz + kch, (size_t)kch, 0.0f);
    wunet_half* const whp = wpk.h();
    wunet_half* const wlp = wpk.h() + wh_halfs;
    int rc = op_split_operand(x, B, kch, L, xs, xslot, oz, oz + kch, bf, st);
    if (rc) return rc;
    {
        ScaleTable T{};
        T.d[0].w = w; T.d[0].wn = (unsigned)((size_t)Cout * Cin * K); T.d[0].gamma = oz; T.d[0].beta = oz; T.d[0].C = 1; T.d[0].sqrtn = 0.0f;
        T.wmax = wmax; T.slots = wslot; T.training = 0;          // (clears wslot[4], which nothing reads)
        WUNET_LAUNCH(h3_scales_kernel, dim3(WUNET_WMAX_PARTS, 1), dim3(WUNET_THREADS), 0, st, T);
        PackH3Table tab{};
        PackH3Desc& d = tab.d[0];
        d.w = w; d.hi = whp; d.lo = wlp; d.Cout = Cout; d.Cin = Cin; d.taps = K; d.rows = rows; d.kch = kch; d.mtiles = p.mtp; d.nch = p.nch;
        d.ntt = p.ntt; d.nfull = ((kch + 7) / 8) / 4; d.ns = h3_stage_count(kch, K, p.ntt);
        d.transposed = transposed; d.wmax = wmax; d.wsc = wslot + 2; d.bf = bf;
        WUNET_LAUNCH(pack_h3_kernel, dim3(64, 1), dim3(WUNET_THREADS), 0, st, tab);
    }
    const bool split = p.ksplit > 1;
    ConvH3Launch h{};
    h.taps = K; h.mrep = p.mrep; h.mtiles_p = p.mtp; h.sps = p.sps; h.nch = p.nch; h.ntt = p.ntt;
    h.B = B; h.rows = rows; h.kch = kch; h.L = L; h.bf = bf;
    h.xh = xs.h(); h.xl = xs.l(); h.zpad = xs.zpad(); h.wh = whp; h.wl = wlp;
    h.bias = split ? nullptr : bias; h.sc = xslot; h.sc2 = wslot + 2; h.out = split ? part.f() : out;
    rc = launch_conv_h3(h, st);
    if (!rc && split) {
        const unsigned blocks = capped_blocks(nout, WUNET_THREADS, 2048);
        const float* partp = part.f();
        const int ks = p.ksplit;
        char pname[48];
        snprintf(pname, sizeof pname, "split_sum_kernel<%d>", ks);          // (profiler: the tests read the split count off the name)
        prof_begin(st, pname, 0.0, 4.0 * (ks + 1.0) * nout);
        WUNET_LAUNCH(split_sum_kernel, dim3(blocks), dim3(WUNET_THREADS), 0, st, partp, ks, nout, out, bias, rows, ilog2(L));
        prof_end(st);
    }
    hipStreamSynchronize(st);
    if (rc) return rc;
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}

int op_wgrad_split_common(const float* gz, const float* x, float* dw, int B, int Cin, int Cout, int L, int K, int bf, hipStream_t st)
{
    LayerGeom l{};
    l.cin = Cin; l.cout = Cout; l.taps = K; l.L = L; l.logL = ilog2(L);
    const H3WgradPlan w = plan_h3_wgrad(B, L, Cin, Cout, K, bf, read_plan_switches());
    SplitBuf xs, gs;
    DevBuf misc, part;
    const int cmax = Cin > Cout ? Cin : Cout;
    // misc: slot of g_z | slot of x | ones | zeros
    if (!misc.alloc((16 + 2 * (size_t)cmax) * sizeof(float)) || !part.alloc((size_t)w.ksplit * h3w_part_stride(l, w) * sizeof(float)))
        return fail(WUNET_E_RUNTIME, "hipMalloc");
    float* gslot = misc.f(), *xslot = misc.f() + 8, *oz = misc.f() + 16;
    WUNET_LAUNCH(fill_kernel, dim3(4), dim3(WUNET_THREADS), 0, st, oz, (size_t)cmax, 1.0f);
    WUNET_LAUNCH(fill_kernel, dim3(4), dim3(WUNET_THREADS), 0, st, oz + cmax, (size_t)cmax, 0.0f);
    int rc = op_split_operand(gz, B, Cout, L, gs, gslot, oz, oz + cmax, bf, st);
    if (!rc) rc = op_split_operand(x, B, Cin, L, xs, xslot, oz, oz + cmax, bf, st);
    if (!rc) rc = launch_wgrad_h3(l, w, xs.h(), xs.l(), gs.h(), gs.l(), gslot, xslot, part.f(), B, st, bf);
    if (!rc) {
        WgradH3ReduceArgs ra{};
        ra.part = part.f(); ra.part_stride = h3w_part_stride(l, w); ra.splits = w.ksplit; ra.dw = dw;
        ra.Cout = Cout; ra.Cin = Cin; ra.taps = K; ra.mrep = w.mrep; ra.tw = K == 15 ? 8 : 5;
        ra.nblocks = w.nblocks; ra.mblocks = w.mblocks; ra.cib = K == 15 ? 32 : 64;
        WUNET_LAUNCH(wgrad_h3_reduce_kernel, dim3(capped_blocks(ra.part_stride / 4, 16, 4096)), dim3(WUNET_THREADS), 0, st, ra);
    }
    hipStreamSynchronize(st);
    if (rc) return rc;
    WUNET_CHECK_LAUNCH();
    return WUNET_OK;
}
}  // namespace

int wunet_op_conv1d_split(const float* x, const float* w, const float* bias, float* z, int B, int Cin, int Cout, int L, int K, void* stream)
{
    if (op_split_check(B, Cin, Cout, L, K, false)) return WUNET_E_ARG;
    return op_conv_split_common(x, w, bias, z, B, Cin, Cout, Cout, Cin, L, K, 0, 0, (hipStream_t)stream);
}

int wunet_op_conv1d_dgrad_split(const float* gz, const float* w, float* dx, int B, int Cin, int Cout, int L, int K, void* stream)
{
    if (op_split_check(B, Cin, Cout, L, K, true)) return WUNET_E_ARG;
    return op_conv_split_common(gz, w, nullptr, dx, B, Cout, Cin, Cout, Cin, L, K, 1, 0, (hipStream_t)stream);
}

int wunet_op_conv1d_wgrad_split(const float* gz, const float* x, float* dw, int B, int Cin, int Cout, int L, int K, void* stream)
{
    if (op_split_check(B, Cin, Cout, L, K, true)) return WUNET_E_ARG;
    return op_wgrad_split_common(gz, x, dw, B, Cin, Cout, L, K, 0, (hipStream_t)stream);
}

int wunet_op_conv1d_bf16(const float* x, const float* w, const float* bias, float* z, int B, int Cin, int Cout, int L, int K, void* stream)
{
    if (op_split_check(B, Cin, Cout, L, K, false)) return WUNET_E_ARG;
    return op_conv_split_common(x, w, bias, z, B, Cin, Cout, Cout, Cin, L, K, 0, 1, (hipStream_t)stream);
}

int wunet_op_conv1d_dgrad_bf16(const float* gz, const float* w, float* dx, int B, int Cin, int Cout, int L, int K, void* stream)
{
    if (op_split_check(B, Cin, Cout, L, K, true)) return WUNET_E_ARG;
    return op_conv_split_common(gz, w, nullptr, dx, B, Cout, Cin, Cout, Cin, L, K, 1, 1, (hipStream_t)stream);
}

int wunet_op_conv1d_wgrad_bf16(const float* gz, const float* x, float* dw, int B, int Cin, int Cout, int L, int K, void* stream)
{
    if (op_split_check(B, Cin, Cout, L, K, true)) return WUNET_E_ARG;
    return op_wgrad_split_common(gz, x, dw, B, Cin, Cout, L, K, 1, (hipStream_t)stream);
}

}  // extern "C"
