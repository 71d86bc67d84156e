/*
 * C ABI of the MI355X-native Wave-U-Net hot path (libwunet_hip.so, gfx950).
 *
 * The reference (haoxiangsnr/Wave-U-Net-for-Speech-Enhancement) is pure Python: its "FFI" for
 * this path is torch's dispatcher.  These entry points are what a maintainer binds instead
 * (ctypes stub in INTEGRATION.md); each cites the reference interface it replaces.
 * All pointers are DEVICE pointers (hipMalloc'ed / torch caching allocator) unless noted, fp32,
 * layout (batch, channel, sample) contiguous.  `stream` is a hipStream_t (NULL = default stream).
 * Every function returns 0 on success and a negative code on failure; wunet_last_error() gives text.
 * Nothing here synchronises the stream: calls only enqueue kernels.
 *
 * Parameter order ("canonical order", == nn.Module.parameters() order of the reference Model,
 * model/unet_basic.py:33-75): for each conv layer in forward order
 * [encoder.0 .. encoder.n-1, middle, decoder.0 .. decoder.n-1]:
 *   conv.weight [Cout,Cin,K], conv.bias [Cout], bn.weight [Cout], bn.bias [Cout];
 * then out.0.weight [1,ci+1,1], out.0.bias [1].   -> 4*(2n+1)+2 pointers.
 * Running statistics: 2*(2n+1) pointers (running_mean, running_var per layer);
 * num_batches_tracked: (2n+1) int64 device pointers.
 */
#ifndef WUNET_HIP_H
#define WUNET_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wunet_ctx wunet_ctx;

#define WUNET_OK 0
#define WUNET_E_ARG (-1)        /* bad argument / unsupported shape */
#define WUNET_E_RUNTIME (-2)    /* HIP runtime error */

#define WUNET_LOSS_MSE 0        /* model/loss.py:3-4  torch.nn.MSELoss()      */
#define WUNET_LOSS_L1 1         /* model/loss.py:6-7  torch.nn.L1Loss()       */
#define WUNET_LOSS_SMOOTH_L1 2  /* torch.nn.SmoothL1Loss(beta=1), SURVEY.md §0 */
#define WUNET_LOSS_SI_SDR 3     /* scale-invariant SDR per row; wunet_loss_rows_* only (no reference counterpart) */
#define WUNET_LOSS_SNR 4        /* SNR per row; wunet_loss_rows_* only (no reference counterpart) */

const char* wunet_last_error(void);

/* Replaces Model.__init__ shape bookkeeping (model/unet_basic.py:33-75) for one (batch, length).
 * length >= 4 and divisible by 2^n_layers, as model/unet_basic.py:86,93 requires (levels of 1-2 samples take a scalar path).  The
 * kernels index rows with shifts and masks: a length that is not a power of two (m * 2^k) is carried in rows padded to the next
 * power of two inside the workspace (zeros where a conv reads the padding, none of it in the BatchNorm statistics, no gradient
 * for it, the upsample at the coordinates of the lengths that exist); the caller's tensors keep their own [B][1][length] layout.
 * Host-side object, no device memory. */
int wunet_create(int n_layers, int channels_interval, int batch, int length, wunet_ctx** out);
void wunet_destroy(wunet_ctx* ctx);

/* GEMM arithmetic of the levels >= 16 samples.  enable = 1: forward convs, data gradients and weight
 * gradients run as fp16-split GEMMs - every fp32 operand x is carried as hi + lo in fp16 (22 significant bits; weights,
 * activations and gradients each with a power-of-two scale derived on the device, so the result does not depend on the
 * magnitude of the checkpoint), a product is three v_mfma_f32_16x16x32_f16 passes with fp32 accumulation -
 * wherever the position grid fills the chip (levels >= 256 samples; 128 .. 16 samples at >= 1024 positions per level,
 * with split-K); 2: wherever the kernels can run (>= 16 samples; small test shapes); 0: fp32 MFMA
 * (v_mfma_f32_16x16x4_f32) everywhere.  Accuracy of the split path is at the fp32 noise floor, but the
 * arithmetic is not bit-identical to the fp32 path.  3 / 4: the layer sets of 1 / 2 in the bf16 mode of the same kernels -
 * operands stored as one bf16 word, one v_mfma_f32_16x16x32_bf16 pass, fp32 accumulation (BASELINE.json configs[4]; accuracy
 * is that of bf16: ~1e-2, tests/test_bf16_mode.py).  A new ctx starts with 0; the Python Engine turns 1 on unless
 * WUNET_H3 says otherwise.  Changes the workspace size: call before wunet_workspace_bytes.  No reference counterpart. */
int wunet_set_h3(wunet_ctx* ctx, int enable);

/* Per-layer BatchNorm mode for the following wunet_forward (training != 0) and wunet_backward* calls on this ctx.
 * frozen: host array of wunet_num_conv_layers(ctx) bytes, non-zero = that layer's BatchNorm uses the running statistics
 * (nn.BatchNorm1d in eval mode) and leaves them untouched; NULL = none (the default).  Host-side only, capture-safe:
 * the values become kernel arguments at enqueue time.  A backward must run under the mask of its forward.
 * Does not change wunet_workspace_bytes. */
int wunet_set_bn_frozen(wunet_ctx* ctx, const unsigned char* frozen, int count);

/* Bytes of device workspace the caller must provide to wunet_forward (with_backward=0: inference;
 * with_backward=1: also holds everything wunet_backward needs). */
size_t wunet_workspace_bytes(const wunet_ctx* ctx, int with_backward);

/* Replaces Model.forward (model/unet_basic.py:77-100).
 * training != 0: BatchNorm uses batch statistics and updates running_mean/var (momentum 0.1,
 * unbiased variance) and num_batches_tracked in place; otherwise running statistics are used.
 * save_for_backward: bit 0 (WUNET_FWD_SAVE, needs a with_backward=1 workspace): additionally keeps what wunet_backward
 * needs - the raw conv outputs, BN statistics and each conv's activated input.
 * Bit 1 (WUNET_FWD_PACKS_VALID, eval mode only): the caller asserts that `workspace` is the one the previous eval-mode wunet_forward of
 * this ctx ran on and that no conv weight has changed since - the weight packs and weight scales it holds are reused and the three
 * pack launches are skipped (enhancement.py:57-69 runs the same weights over every chunk of every file; engine.Engine keys this on the
 * parameters' addresses and autograd version counters). */
#define WUNET_FWD_SAVE 1
#define WUNET_FWD_PACKS_VALID 2
int wunet_forward(wunet_ctx* ctx, const float* noisy, const float* const* params,
                  float* const* running, long long* const* num_batches_tracked, int training,
                  int save_for_backward, void* workspace, float* enhanced, void* stream);

/* Replaces autograd's backward of Model.forward (trainer/trainer.py:37 loss.backward()).
 * Must follow a training-mode wunet_forward on the same ctx/workspace/params/noisy.
 * grad_enhanced: dL/d(enhanced) [B,1,T].  grads: same shapes/order as params; every tensor is
 * overwritten (conv biases feeding a batch-statistics BatchNorm get an exact 0; a layer frozen by wunet_set_bn_frozen gets
 * its true bias gradient).  The gradient with respect to `noisy` is a separate call: wunet_backward_input. */
int wunet_backward(wunet_ctx* ctx, const float* noisy, const float* const* params,
                   const float* enhanced, const float* grad_enhanced, void* workspace,
                   float* const* grads, void* stream);
/* Same as wunet_backward but only runs conv layers [layer_begin, layer_end) in backward order
 * (layer index in forward order; the output head belongs to layer 2n).  Lets the caller overlap the
 * RCCL all-reduce of finished gradient buckets with the remaining layers. */
int wunet_backward_range(wunet_ctx* ctx, const float* noisy, const float* const* params,
                         const float* enhanced, const float* grad_enhanced, void* workspace,
                         float* const* grads, int layer_begin, int layer_end, void* stream);
/* wunet_backward_range without the final "caller's stream waits for the weight-gradient stream": the next range's
 * data-gradient chain is not held up at the bucket boundary.  The weight gradients of the range are complete for a stream
 * after wunet_backward_join(ctx, that_stream) - e.g. the stream the RCCL all-reduce of the bucket is enqueued from.  The range
 * with layer_begin == 0 (the end of the backward) always joins `stream`.  The side stream is per (ctx, device): a ctx may be
 * used from several devices / threads at once as long as each call runs with its device current. */
int wunet_backward_range_async(wunet_ctx* ctx, const float* noisy, const float* const* params,
                               const float* enhanced, const float* grad_enhanced, void* workspace,
                               float* const* grads, int layer_begin, int layer_end, void* stream);
int wunet_backward_join(wunet_ctx* ctx, void* stream);
/* autograd's gradient with respect to the waveform input of Model.forward (model/unet_basic.py:77-100): grad_noisy [B,1,T]
 * receives dL/d(noisy) and is overwritten.  Must follow the backward call that covers layer 0 (wunet_backward, or the _range /
 * _range_async call with layer_begin == 0) with the same ctx, workspace, params, frozen mask and stream, before the next forward on
 * that workspace: it reads what that backward left in the workspace (the head gradient, encoder.0's gradient or the data gradients
 * it is rebuilt from).  Capture-safe: no allocation, no synchronisation, no host read-back.  Changes nothing else - parameter
 * gradients, running statistics and the workspace size are those of the backward alone.  No reference counterpart (the reference
 * gets it from autograd). */
int wunet_backward_input(wunet_ctx* ctx, const float* noisy, const float* const* params, void* workspace,
                         float* grad_noisy, void* stream);

/* Replaces loss_function(clean, enhanced) (trainer/trainer.py:36; model/loss.py:3-7), mean reduction.
 * scratch: >= wunet_loss_scratch_bytes() device bytes.  loss_out: device float. */
size_t wunet_loss_scratch_bytes(void);
int wunet_loss_forward(int kind, const float* clean, const float* enhanced, size_t n,
                       float* loss_out, void* scratch, void* stream);
/* grad_enhanced[i] = grad_loss[0] * d loss / d enhanced[i]  (grad_loss: device float, usually 1). */
int wunet_loss_backward(int kind, const float* clean, const float* enhanced, const float* grad_loss,
                        size_t n, float* grad_enhanced, void* stream);

/* Row losses: scale-invariant SDR (Le Roux et al., "SDR - half-baked or well done?") and plain SNR per utterance, the criterion and
 * the validation score of speech enhancement.  No reference counterpart (model/loss.py has the two element-wise means only).
 * clean = s and enhanced = e are [rows][row_len]; zero_mean != 0 removes each row's own mean from s and from e first.  Per row, with
 * p = <e,s>, q = <s,s>, r = <e,e>:
 *   WUNET_LOSS_SI_SDR: alpha = p / (q + eps), Et = alpha^2 q, En = r - 2 alpha p + alpha^2 q (= |e - alpha s|^2, not below 0)
 *   WUNET_LOSS_SNR:    Et = q, En = sum (e - s)^2 accumulated from the differences
 *   v = 10 log10((Et + eps) / (En + eps)) [dB];  loss_out = -(1 / rows) sum v.
 * One pass over the pair; every sum and everything derived from it is double, only the outputs are rounded to float; fixed
 * summation order, no atomics: bit-identical run to run.  per_row_db (NULL or [rows]) receives v.  coefs (NULL when no backward
 * follows, else [rows * WUNET_LOSS_ROW_COEFS] doubles) receives A, C, D, v, mx, ms per row with dv/d e[i] = A e[i] + C s[i] + D;
 * mx / ms are the row means that were removed (of e, or of e - s for SNR, and of s; 0 without zero_mean), D = -A mx - C ms.
 * scratch: >= wunet_loss_rows_scratch_bytes(rows, row_len) device bytes, no memset needed.  The backward (same kind as the forward)
 * writes grad_enhanced[i] = grad_loss[0] * (-1 / rows) * (A e[i] + C s[i] + D), applied in double in its centred form
 * A (e[i] - mx) + C (s[i] - ms) and rounded once: a sample at its row's mean gets an exact 0.
 * Caller-owned memory, no allocation, no synchronisation, no host read-back: both calls can be captured.  Pointers need 4-byte
 * alignment only (16-byte loads where clean, enhanced and the gradient agree modulo 16).
 * wunet_loss_forward / wunet_loss_backward keep refusing these two kinds. */
#define WUNET_LOSS_ROW_COEFS 6   /* A, C, D, v, mx, ms per row, double */
size_t wunet_loss_rows_scratch_bytes(size_t rows, size_t row_len);
int wunet_loss_rows_forward(int kind, int zero_mean, double eps, const float* clean, const float* enhanced,
                            size_t rows, size_t row_len, float* loss_out, float* per_row_db, double* coefs,
                            void* scratch, void* stream);
int wunet_loss_rows_backward(int kind, const float* clean, const float* enhanced, const double* coefs, const float* grad_loss,
                             size_t rows, size_t row_len, float* grad_enhanced, void* stream);

/* Multi-resolution STFT loss (Yamamoto et al., "Parallel WaveGAN"): spectral convergence plus log-magnitude L1.  No reference
 * counterpart (the reference only looks at STFT magnitudes in its validation epoch, trainer/trainer.py:108-110, on the host).
 * One resolution (n_fft = N, hop = H, win_length = W <= N) of clean = c and enhanced = e, both [rows][row_len = T]:
 *   window   periodic Hann of length W, w[j] = 0.5 - 0.5 cos(2 pi j / W), zero-padded to N with (N - W) / 2 zeros on the left;
 *   framing  center=True, pad_mode="reflect": x_pad[j] = x[reflect(j - N/2)], frames f = 0 .. T / H (F = 1 + T / H); needs N/2 <= T - 1;
 *   spectrum X[f][b] = sum_k w[k] x_pad[f H + k] exp(-2 pi i k b / N), b = 0 .. N/2;  P = re^2 + im^2,  S = sqrt(max(P, clamp));
 *   sc  = sqrt(sum (S_c - S_e)^2) / sqrt(sum S_c^2),  mag = mean |ln S_c - ln S_e|, both over all rows, frames and bins;
 *   loss = (1 / n_res) sum_i (sc_weight sc_i + mag_weight mag_i).
 * Gradient with respect to `enhanced` only.  It follows torch.clamp: a bin with P_e < clamp passes no gradient.  ONE departure from
 * autograd: where sum (S_c - S_e)^2 == 0 the sc term contributes 0 instead of NaN.
 * Supported: 16 <= N <= 4096 with N % 16 == 0, 1 <= H <= N, 1 <= W <= N, clamp > 0; anything else is WUNET_E_ARG with a message.
 * Arithmetic: fp32 operands and fp32 MFMA accumulation against a basis computed in double and rounded once; every reduction and
 * coefficient in double; no atomics, every sum has one fixed order: bit-identical run to run.
 * The calls of one loss:
 *   once per (N, W): wunet_stft_basis into wunet_stft_basis_bytes(N) bytes (16-byte aligned);
 *   per resolution:  wunet_stft_forward(clean, enhanced, ..) writes its partial sums to `scratch` (>= wunet_stft_scratch_bytes(..)),
 *                    and, when `saved` is given (>= wunet_stft_saved_bytes(..)), re_e, im_e and S_c for the backward; mag_out (NULL or
 *                    [rows * F][N/2 + 1]) receives S_e.  clean == NULL: the magnitudes of `enhanced` alone into mag_out (scratch and
 *                    saved unused, clamp >= 0) - the metric path;
 *   once:            wunet_stft_finalize over the TABLE of the resolutions' scratch buffers (host arrays of n_res <=
 *                    WUNET_STFT_MAX_RESOLUTIONS entries, read during the call): the loss, accumulated over the resolutions in double
 *                    and rounded once, and coefs[n_res][WUNET_STFT_COEFS] = a, b, sc, mag with
 *                    a = sc_weight / (n_res |S_c - S_e| |S_c|), b = mag_weight / (n_res rows F bins);
 *   per resolution:  wunet_stft_backward(saved, coefs + i * WUNET_STFT_COEFS, grad_loss, ..): the adjoint GEMM into `scratch`
 *                    (>= wunet_stft_scratch_bytes(.., with_backward = 1); the forward's buffer may be reused after the finalize), then
 *                    the overlap-add as a gather; grad_enhanced = (accumulate ? grad_enhanced : 0) + grad_loss[0] * d loss_i / d e,
 *                    so several resolutions sum in the order of the calls.
 * Caller-owned memory, no allocation, no synchronisation, no host read-back: every call can be captured. */
#define WUNET_STFT_MAX_RESOLUTIONS 8
#define WUNET_STFT_COEFS 4       /* a, b, sc, mag per resolution, double */
size_t wunet_stft_basis_bytes(int n_fft);
int wunet_stft_basis(int n_fft, int win_length, float* basis, void* stream);
size_t wunet_stft_scratch_bytes(size_t rows, size_t row_len, int n_fft, int hop, int with_backward);
size_t wunet_stft_saved_bytes(size_t rows, size_t row_len, int n_fft, int hop);
int wunet_stft_forward(const float* clean, const float* enhanced, size_t rows, size_t row_len, int n_fft, int hop, int win_length,
                       double clamp, const float* basis, void* scratch, float* saved, float* mag_out, void* stream);
int wunet_stft_finalize(int n_res, const void* const* scratch, size_t rows, size_t row_len, const int* n_fft, const int* hop,
                        double sc_weight, double mag_weight, float* loss_out, double* coefs, void* stream);
int wunet_stft_backward(const float* saved, const double* coefs, const float* grad_loss, size_t rows, size_t row_len, int n_fft, int hop,
                        int win_length, double clamp, const float* basis, void* scratch, float* grad_enhanced, int accumulate,
                        void* stream);

/* Power-law compressed spectral loss with a complex (phase-aware) term (Braun & Tashev 2021, "A consolidated view of loss functions
 * for supervised deep learning-based speech enhancement"; the DNS-challenge baseline loss).  No reference counterpart.  One
 * resolution (N, H, W) frames and transforms clean = c and enhanced = e exactly as the STFT loss above does (same window, centring,
 * reflect padding, frames f = 0 .. T / H, bins b = 0 .. N/2, N/2 <= T - 1, and the basis of wunet_stft_basis).  Per bin of either signal:
 *   P = re^2 + im^2,  Pc = max(P, clamp),  A = Pc^(compress / 2),  Z = (re + i im) Pc^((compress - 1) / 2);
 *   L_i = mean over rows, frames and bins of (1 - complex_weight) (A_c - A_e)^2 + complex_weight |Z_c - Z_e|^2;
 *   loss = (1 / n_res) sum_i L_i.
 * Gradient with respect to `enhanced` only.  It follows torch.clamp: where P_e < clamp the factors Pc^.. are constants - A_e passes no
 * gradient and Z_e is linear in (re, im), so an all-zero enhanced row gets a finite, non-zero gradient.  Equal signals give exactly 0
 * and an all-zero gradient.
 * Supported: the STFT loss's N / H / W, 1 .. WUNET_STFT_MAX_RESOLUTIONS resolutions, 0 < compress <= 1, 0 <= complex_weight <= 1, clamp
 * finite and > 0; anything else is WUNET_E_ARG with a message.
 * Arithmetic: fp32 operands and fp32 MFMA accumulation against the STFT loss's basis; the per-bin powers in double, A and Z rounded to
 * float32 once (the backward recomputes the enhanced side to the same bits); every reduction and coefficient in double; no atomics,
 * every sum has one fixed order: bit-identical run to run.
 * The calls of one loss (the buffers' byte sizes are passed and checked: a buffer sized for another resolution is refused):
 *   per resolution:  wunet_cspec_forward writes its partial sums to `scratch` (scratch_bytes >= wunet_cspec_scratch_bytes(..)) and, when
 *                    `saved` is given (saved_bytes == wunet_cspec_saved_bytes(..); else NULL and 0), five planes [rows * F][BP] for the
 *                    backward: re_e, im_e, A_c, Re Z_c, Im Z_c;
 *   once:            wunet_cspec_finalize over the TABLE of the resolutions' scratch buffers (host arrays of n_res entries, read during
 *                    the call): the loss, accumulated over the resolutions in double and rounded once, and (coefs != NULL)
 *                    coefs[n_res][WUNET_CSPEC_COEFS] = (1 - complex_weight) / (n_res count), complex_weight / (n_res count), the mean
 *                    of (A_c - A_e)^2, the mean of |Z_c - Z_e|^2, with count = rows F bins;
 *   per resolution:  wunet_cspec_backward(saved, .., coefs + i * WUNET_CSPEC_COEFS, grad_loss, ..): the adjoint GEMM into `scratch`
 *                    (scratch_bytes >= wunet_cspec_scratch_bytes(.., with_backward = 1); the forward's buffer may be reused after the
 *                    finalize), then the STFT loss's overlap-add; grad_enhanced = (accumulate ? grad_enhanced : 0) + grad_loss[0] *
 *                    d loss_i / d e, so several resolutions sum in the order of the calls.  compress and clamp: the forward's.
 * Caller-owned memory, no allocation, no synchronisation, no host read-back: every call can be captured. */
#define WUNET_CSPEC_COEFS 4      /* two gradient scales, two term values per resolution, double */
size_t wunet_cspec_scratch_bytes(size_t rows, size_t row_len, int n_fft, int hop, int with_backward);
size_t wunet_cspec_saved_bytes(size_t rows, size_t row_len, int n_fft, int hop);
int wunet_cspec_forward(const float* clean, const float* enhanced, size_t rows, size_t row_len, int n_fft, int hop, int win_length,
                        double compress, double clamp, const float* basis, void* scratch, size_t scratch_bytes, float* saved,
                        size_t saved_bytes, void* stream);
int wunet_cspec_finalize(int n_res, const void* const* scratch, size_t rows, size_t row_len, const int* n_fft, const int* hop,
                         double complex_weight, float* loss_out, double* coefs, void* stream);
int wunet_cspec_backward(const float* saved, size_t saved_bytes, const double* coefs, const float* grad_loss, size_t rows, size_t row_len,
                         int n_fft, int hop, int win_length, double compress, double clamp, const float* basis, void* scratch,
                         size_t scratch_bytes, float* grad_enhanced, int accumulate, void* stream);

/* Multi-scale log-mel spectrogram loss (HiFi-GAN's mel loss; the multi-scale mel loss of DAC / EnCodec-style codecs).  No reference
 * counterpart.  One resolution (N, H, W) frames and transforms clean = c and enhanced = e exactly as the STFT loss above does (same
 * window, centring, reflect padding, frames f = 0 .. T / H, bins b = 0 .. N/2, N/2 <= T - 1, and the basis of wunet_stft_basis).  With a
 * filterbank filt = Phi [n_mels][BP] (BP = N/2 + 1 rounded up to 32; non-negative float32, the padding columns 0, 16-byte aligned; the
 * library knows nothing of mel scales - any non-negative bank will do):
 *   P = re^2 + im^2,  Pc = max(P, clamp),  S = Pc^(power / 2),  m[f][j] = sum_b Phi[j][b] S[f][b],  l = ln max(m, floor);
 *   L_i = mean over rows, frames and j of log_weight |l_c - l_e| + lin_weight |m_c - m_e|;
 *   loss = (1 / n_res) sum_i L_i.
 * Gradient with respect to `enhanced` only: autograd's of this graph with torch.clamp and abs - it passes where P_e >= clamp and where
 * m_e >= floor, sign(0) = 0.  Equal signals give exactly 0 and an all-zero gradient; an all-zero row of Phi adds nothing to the sums
 * and still counts in the mean.
 * Supported: the STFT loss's N / H / W, 1 .. WUNET_STFT_MAX_RESOLUTIONS resolutions, 1 <= n_mels <= WUNET_MEL_MAX_FILTERS, power 1 or 2,
 * clamp and floor finite and > 0 (>= 0 for the call without `clean`), the weights finite and >= 0 and not both 0; anything else is
 * WUNET_E_ARG with a message.
 * Arithmetic: fp32 operands and fp32 MFMA accumulation in both GEMMs of either direction; the logs, every reduction and every
 * coefficient in double; no atomics, every sum has one fixed order: bit-identical run to run.
 * The calls of one loss (the buffers' byte sizes are passed and checked; scratch and saved 16-byte aligned):
 *   per resolution:  wunet_mel_forward writes its partial sums and the planes S_e, S_c to `scratch` (scratch_bytes >=
 *                    wunet_mel_scratch_bytes(..)) and, when `saved` is given (saved_bytes == wunet_mel_saved_bytes(..); else NULL and
 *                    0), re_e, im_e [rows * F][BP] and m_c, m_e [rows * F][MP] (MP = n_mels rounded up to 16) for the backward; the
 *                    buffer also holds the plane the backward writes dS to.  mel_out must be NULL.  clean == NULL: the mel spectrogram
 *                    of `enhanced` alone into mel_out [rows * F][n_mels] - m, or ln max(m, floor) where floor > 0 (saved NULL and 0;
 *                    scratch as above) - the metric path;
 *   once:            wunet_mel_finalize over the TABLE of the resolutions' scratch buffers (host arrays of n_res entries, read during
 *                    the call): the loss, accumulated over the resolutions in double and rounded once, and (coefs != NULL)
 *                    coefs[n_res][WUNET_MEL_COEFS] = log_weight / (n_res count), lin_weight / (n_res count), the mean of |l_c - l_e|,
 *                    the mean of |m_c - m_e|, with count = rows F n_mels;
 *   per resolution:  wunet_mel_backward(saved, .., coefs + i * WUNET_MEL_COEFS, grad_loss, ..): the transposed projection dS = g Phi
 *                    into `saved`, the adjoint GEMM into `scratch` (scratch_bytes >= wunet_mel_scratch_bytes(.., with_backward = 1); the
 *                    forward's buffer may be reused after the finalize), then the STFT loss's overlap-add; grad_enhanced =
 *                    (accumulate ? grad_enhanced : 0) + grad_loss[0] * d loss_i / d e, so several resolutions sum in the order of the
 *                    calls.  filt, power, clamp and floor: the forward's.
 * Caller-owned memory, no allocation, no synchronisation, no host read-back: every call can be captured. */
#define WUNET_MEL_MAX_FILTERS 128
#define WUNET_MEL_COEFS 4        /* two gradient scales, two term values per resolution, double */
size_t wunet_mel_scratch_bytes(size_t rows, size_t row_len, int n_fft, int hop, int with_backward);
size_t wunet_mel_saved_bytes(size_t rows, size_t row_len, int n_fft, int hop, int n_mels);
int wunet_mel_forward(const float* clean, const float* enhanced, size_t rows, size_t row_len, int n_fft, int hop, int win_length, int n_mels,
                      const float* filt, int power, double clamp, double floor, const float* basis, void* scratch, size_t scratch_bytes,
                      float* saved, size_t saved_bytes, float* mel_out, void* stream);
int wunet_mel_finalize(int n_res, const void* const* scratch, size_t rows, size_t row_len, const int* n_fft, const int* hop,
                       const int* n_mels, double log_weight, double lin_weight, float* loss_out, double* coefs, void* stream);
int wunet_mel_backward(float* saved, size_t saved_bytes, const double* coefs, const float* grad_loss, size_t rows, size_t row_len, int n_fft,
                       int hop, int win_length, int n_mels, const float* filt, int power, double clamp, double floor, const float* basis,
                       void* scratch, size_t scratch_bytes, float* grad_enhanced, int accumulate, void* stream);

/* STOI per row(no reference counterpart on the device: the reference's validation epoch calls pystoi on the host per recording,
 * trainer/trainer.py:128-143, util/utils.py:116-117): Taal et al. 2011 with pystoi's choices for stoi(clean, estimate, fs,
 * extended=False) - resample_poly to 10 kHz with pystoi's Kaiser filter, removal of the frames (256 / hop 128, hanning(258)[1:-1])
 * more than 40 dB below the clean row's loudest, 512-point spectra of the overlap-added rest, 15 third-octave bands from 150 Hz,
 * clipped and normalised correlations over all segments of 30 frames, their mean.  Fewer than 30 spectral frames (a row_len too short
 * for one frame included): the score 1e-5, pystoi's value.
 *   wunet_stoi_tables_bytes(fs): bytes of the per-rate tables (0: fs refused - fs <= 0, or a rate whose filter needs more than 4096
 *     taps, i.e. max(p, q) > 56 for 10000 / fs = p / q in lowest terms; 8, 12, 16, 20, 24, 32 and 48 kHz all fit).
 *   wunet_stoi_tables_build: the windowed 512-point DFT basis, the window and the resampler's taps into `tables` (16-byte aligned).
 *     taps: DEVICE pointer to the n_taps = 2 L + 1 float32 filter taps (L = ceil(52 / (28.714 fc / 10)), fc = 1 / (2 max(p, q)),
 *     h[t] = kaiser(2 L + 1, 0.1102 (60 - 8.7))[t + L] 2 p fc sinc(2 fc t), normalised to sum 1; computed by the caller in double);
 *     n_taps = 0 and taps = NULL at fs = 10000.
 *   wunet_stoi_forward: out[row] (float32) and, when frames_out != NULL, the spectral frame count of every row (int32).  scratch:
 *     >= wunet_stoi_scratch_bytes(rows, row_len, fs) device bytes, 16-byte aligned, no memset needed; the waveforms need 4-byte
 *     alignment only.  rows <= 65535.
 * Every sum in double and in one fixed order, no atomics: bit-identical run to run.  Caller-owned memory, no allocation, no
 * synchronisation, no host read-back (the per-row frame counts stay in device memory): every call can be captured. */
size_t wunet_stoi_tables_bytes(int fs);
int wunet_stoi_tables_build(int fs, const float* taps, size_t n_taps, float* tables, void* stream);
size_t wunet_stoi_scratch_bytes(size_t rows, size_t row_len, int fs);
int wunet_stoi_forward(const float* clean, const float* estimate, size_t rows, size_t row_len, int fs, const float* tables, void* scratch,
                       float* out, int* frames_out, void* stream);

/* STOI as a training loss (Fu et al. 2018, "End-to-end waveform utterance enhancement ... based on STOI"): loss = -(1 / rows) sum_row s_row
 * with s_row the row's score exactly as wunet_stoi_forward defines it - a row with fewer than 30 spectral frames contributes the
 * constant 1e-5 and no gradient - the mean taken in double over the double row scores, in row order, and rounded once.  The tables
 * are those of wunet_stoi_tables_build.
 *   wunet_stoi_loss_forward: the launch sequence of wunet_stoi_forward, which also keeps in `saved`
 *     (>= wunet_stoi_loss_saved_bytes(..)) what the backward needs: the kept-frame table, its inverse and the counts, the band powers of
 *     both signals, re and im of the estimate.  per_row_out (NULL or [rows] float32) receives s_row, frames_out (NULL or [rows] int32)
 *     the spectral frame counts.
 *   wunet_stoi_loss_backward: grad_estimate = grad_loss[0] * d loss / d estimate, written for EVERY sample of every row (rows without
 *     a segment and samples outside every kept frame get exact zeros: no memset needed).  It inverts the chain stage by stage -
 *     segments -> band magnitudes -> adjoint DFT GEMM -> silence-free signal and frames -> transposed resampling filter - each stage a
 *     gather.  Conventions of the derivative:
 *       - the silent-frame mask depends on `clean` only and is a constant; there is no gradient with respect to `clean`;
 *       - min(alpha y, clip x) passes the gradient through alpha y where alpha y < clip x and nothing otherwise; the alpha y branch
 *         includes the dependence of alpha = |x| / (|y| + eps) on every y of the segment;
 *       - ONE departure from autograd: where a band magnitude of the estimate is exactly 0, that (frame, band) passes no gradient
 *         (autograd: NaN - an all-zero estimate gets a zero gradient here).  Likewise a segment whose clipped, centred estimate is all 0
 *         drops the derivative of its norm.  An all-zero clean row gives an all-zero gradient.
 *   scratch: >= wunet_stoi_loss_scratch_bytes(..) device bytes for either call (the two calls may use different buffers), no memset.
 * fp32 operands and fp32 MFMA accumulation, every reduction in double and in one fixed order, no atomics: bit-identical run to run.
 * Caller-owned memory; tables, scratch and saved 16-byte aligned, the waveforms and the gradient 4-byte aligned; no allocation, no
 * synchronisation, no host read-back: both calls can be captured.  rows <= 65535; argument errors are WUNET_E_ARG with a message. */
size_t wunet_stoi_loss_scratch_bytes(size_t rows, size_t row_len, int fs);
size_t wunet_stoi_loss_saved_bytes(size_t rows, size_t row_len, int fs);
int wunet_stoi_loss_forward(const float* clean, const float* estimate, size_t rows, size_t row_len, int fs, const float* tables, void* scratch,
                            void* saved, float* loss_out, float* per_row_out, int* frames_out, void* stream);
int wunet_stoi_loss_backward(const void* saved, const float* grad_loss, size_t rows, size_t row_len, int fs, const float* tables, void* scratch,
                             float* grad_estimate, void* stream);

/* ESTOI per row and as a training loss: the other branch of the same pystoi call, stoi(clean, estimate, fs, extended=True) (Jensen &
 * Taal 2016; as a loss: Kolbaek et al. 2018).  Everything up to the band magnitudes is wunet_stoi_forward's - the same tables
 * (wunet_stoi_tables_build), the same kept-frame rule and frame counts, the same 1e-5 for a row with fewer than 30 spectral frames -
 * and every entry point takes the arguments of its wunet_stoi_* counterpart, in the same order, with the same argument errors.  With
 * X[f][j], Y[f][j] the band magnitudes of the clean row and of the estimate (frame f, band j < 15), every segment m (frames m .. m + 29)
 * normalises its 30 x 15 block of X and, separately, of Y twice:
 *   1. per band j, over the 30 frames: minus the mean, divided by (the 2-norm + EPS);
 *   2. per frame n, over the 15 bands of the result of 1: minus the mean, divided by (the 2-norm + EPS);
 * EPS = 2^-52.  d_m = (1 / 30) sum_n sum_j x~[n][j] y~[n][j]; the row's score is the mean of d_m over its segments; the loss is
 * -(1 / rows) sum_row score_row, the mean taken in double and rounded once, as for wunet_stoi_loss_forward.
 * ONE departure from pystoi: before each normalisation pystoi adds EPS * randn dither to the block, only to avoid 0 / 0.  Nothing is
 * added here; EPS stands in the two denominators instead.  The difference is at the 1e-15 level on any non-degenerate input.
 *   wunet_estoi_forward / wunet_estoi_scratch_bytes: as wunet_stoi_forward / wunet_stoi_scratch_bytes.
 *   wunet_estoi_loss_forward / _saved_bytes: as wunet_stoi_loss_forward; `saved` holds the same things.
 *   wunet_estoi_loss_backward: grad_estimate = grad_loss[0] * d loss / d estimate, written for EVERY sample of every row.  The segment
 *     stage is two launches - every segment's 30 x 15 block d d_m / d Y into scratch, then per (frame, band) the blocks of its at most 30
 *     segments added in segment order - and the adjoint DFT GEMM, the frame gather and the transposed resampler of
 *     wunet_stoi_loss_backward run behind it.  scratch: >= wunet_estoi_loss_scratch_bytes(..) (larger than STOI's by those blocks:
 *     rows * (frames - 29) * 450 doubles).  Conventions of the derivative:
 *       - the silent-frame mask depends on `clean` only and is a constant; there is no gradient with respect to `clean`;
 *       - a band row or a frame column whose centred norm is exactly 0 normalises to zeros and passes no gradient (autograd: NaN);
 *       - a (frame, band) whose Y is exactly 0 passes no gradient, as for wunet_stoi_loss_backward;
 *       - a row with fewer than 30 spectral frames contributes the constant 1e-5 and an all-zero gradient;
 *       - an all-zero estimate scores exactly 0.0 with an all-zero gradient.
 * All segment arithmetic in double and in one fixed order, no atomics: bit-identical run to run.  Alignment, capture and limits as for
 * the wunet_stoi_* calls. */
size_t wunet_estoi_scratch_bytes(size_t rows, size_t row_len, int fs);
int wunet_estoi_forward(const float* clean, const float* estimate, size_t rows, size_t row_len, int fs, const float* tables, void* scratch,
                        float* out, int* frames_out, void* stream);
size_t wunet_estoi_loss_scratch_bytes(size_t rows, size_t row_len, int fs);
size_t wunet_estoi_loss_saved_bytes(size_t rows, size_t row_len, int fs);
int wunet_estoi_loss_forward(const float* clean, const float* estimate, size_t rows, size_t row_len, int fs, const float* tables, void* scratch,
                             void* saved, float* loss_out, float* per_row_out, int* frames_out, void* stream);
int wunet_estoi_loss_backward(const void* saved, const float* grad_loss, size_t rows, size_t row_len, int fs, const float* tables, void* scratch,
                              float* grad_estimate, void* stream);

/* replaces optimizer.step() of torch.optim.Adam(params, lr, betas) as the reference builds it
 * (train.py:31-35; eps, weight_decay=0, amsgrad=False fixed by the reference's call) for n_tensors tensors in one
 * or two launches.  step is the 1-based step count AFTER the increment (torch's state["step"]).  numels: host array.
 * grad_scale multiplies every gradient first (1/world_size of the data-parallel average, trainer/base_trainer.py:26-27, folded
 * into the step).  step_dev != NULL: the step count lives in device memory (int64), is incremented by the call and the bias
 * corrections are computed on the device into hyper_dev (2 floats) - `step` is ignored; this is what makes the whole training
 * step capturable in a hipGraph. */
int wunet_adam_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                    float* const* exp_avg_sq, const size_t* numels, double lr, double beta1, double beta2, double eps,
                    long long step, double grad_scale, long long* step_dev, float* hyper_dev, void* stream);
/* wunet_adam_step with three optional parts, each a per-step scalar in device memory so that a captured step replays unchanged:
 * replaces torch.nn.utils.clip_grad_norm_(params, max_grad_norm) + torch.optim.AdamW(params, lr, betas, eps, weight_decay).step()
 * (no reference counterpart: train.py:31-35 builds a plain Adam and trainer/trainer.py:34-38 does not clip).
 *   max_grad_norm > 0: the 2-norm over ALL n_tensors gradients (after grad_scale) is summed in double by one extra read of the
 *     gradients, clip = min(1, max_grad_norm / (norm + 1e-6)) multiplies every gradient inside the update.  The gradient tensors
 *     are NOT modified (clip_grad_norm_ scales them in place).  A non-finite norm propagates as in torch with
 *     error_if_nonfinite=False.  scratch: >= wunet_adam_scratch_bytes(n_tensors) device bytes, no memset needed.
 *   weight_decay > 0: decoupled, p <- p * (1 - lr * weight_decay) before the update (torch.optim.AdamW's order).
 *   lr_dev != NULL: the learning rate is read from this device double (`lr` is ignored): a scheduler changes the value, the
 *     launches and their arguments stay the same.
 * step_dev may be NULL (then `step` counts, as in wunet_adam_step).  hyper_dev is required, WUNET_ADAM_HYPER_FLOATS floats that
 * the call overwrites: [0] lr / (1 - beta1^t), [1] sqrt(1 - beta2^t), [2] clip (1 when off), [3] the norm before clipping
 * (0 when off), [4] 1 - lr * weight_decay, the rest reserved.  Capture-safe: no allocation, no synchronisation, no host read-back.
 * Both entry points run the same kernels; with all three parts off the result has the bits of wunet_adam_step, which stays the
 * entry for a 2-float hyper buffer (or none): nothing behind its slot 1 is read or written. */
#define WUNET_ADAM_HYPER_FLOATS 8
size_t wunet_adam_scratch_bytes(int n_tensors);
int wunet_adam_step_ex(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                       float* const* exp_avg_sq, const size_t* numels, double lr, double beta1, double beta2, double eps,
                       long long step, double grad_scale, double weight_decay, double max_grad_norm, long long* step_dev,
                       float* hyper_dev, const double* lr_dev, void* scratch, void* stream);

/* Introspection for tests / profiling: float offset of layer i's raw conv output inside the
 * workspace, its channel count and length. */
int wunet_layer_info(const wunet_ctx* ctx, int layer, size_t* z_offset_floats, int* channels, int* length);
int wunet_num_conv_layers(const wunet_ctx* ctx);

/* Optional per-launch timing of the MFMA kernels with HIP events recorded on the launch stream
 * (bench.py's roofline leg; no reference counterpart).  collect() synchronises the device, writes
 * "kernel name\tlaunches\ttotal_ms\ttotal_algorithmic_flops\ttotal_algorithmic_bytes\n" per kernel
 * into buf and clears the records. */
int wunet_profile_enable(int on);
long long wunet_profile_collect(char* buf, size_t cap);
/* Measurement hook (environment WUNET_STAMP=1, otherwise no launches): one-thread kernels write the device's 100 MHz wall clock beside the
 * backward's launches - slot 2 i in front of layer i's data gradient on the caller's stream, slot 2 i + 1 in front of its weight gradient
 * on the library's side stream, slots 126 / 127 where the two chains join.  They are captured into a step graph like any launch, so a graph
 * REPLAY can be asked when its two chains ran without a tracer attached.  Copies up to 128 values of the last backward to `out`. */
int wunet_debug_stamps(unsigned long long* out, int n);

/* ---- data-parallel exchange: the flat fp32 gradient buffer summed over the GPUs of the job by RCCL.
 * Replaces what `torch.nn.DataParallel(model, device_ids=...)` does implicitly per step - replicate / scatter / gather and the
 * reduce-add of the replicas' gradients onto device 0 (/root/reference/trainer/base_trainer.py:26-27) - with ONE process per GPU
 * and an all-reduce (sum) over xGMI; the caller scales by 1/world (or leaves it to wunet_adam_step's grad_scale).
 * wunet_comm_unique_id: rank 0 draws the 128-byte RCCL id; the caller carries it to the other ranks (any side channel: a file, a
 * socket, torch.distributed's store).  wunet_comm_create: collective over all `world` ranks, on the calling thread's current device.
 * wunet_comm_allreduce_sum: in place over buf[0 .. count), enqueued on `stream` like a kernel: it orders with the backward's kernels
 * on that stream and can be captured into the step's hipGraph.  World size 1 needs no RCCL (the sum over one rank is a no-op). */
#define WUNET_COMM_ID_BYTES 128
typedef struct wunet_comm wunet_comm;
int wunet_comm_unique_id(unsigned char* id /* [WUNET_COMM_ID_BYTES] */);
int wunet_comm_create(const unsigned char* id, int world, int rank, wunet_comm** out);
int wunet_comm_allreduce_sum(wunet_comm* comm, float* buf, size_t count, void* stream);
int wunet_comm_world(const wunet_comm* comm);
void wunet_comm_destroy(wunet_comm* comm);

/* SURVEY.md section 8 (f4), the data input path.  Replaces, for a whole batch and on the device, the reference's per-item aligned
 * random crop - `sample_fixed_length_data_aligned(mixture, clean, sample_length)`, /root/reference/util/utils.py:101-113, called from
 * `Dataset.__getitem__`, dataset/waveform_dataset.py:56-67 - and the collate of train.py:15-21: window b of BOTH outputs is
 * samples starts[b] .. starts[b] + length - 1 of the two flat float32 arrays (`total` samples each, resident in HBM; starts = device
 * int64, drawn by the caller with the reference's distribution: uniform over [item_start, item_start + item_length - length]).
 * mixture / clean receive [batch][1][length] float32.  Starts outside [0, total - length] are clamped (never an out-of-range read). */
int wunet_crop_windows(const float* mixture_flat, const float* clean_flat, const long long* starts, long long total,
                       int batch, int length, float* mixture, float* clean, void* stream);

/* Mixtures made on the device (no reference counterpart: the reference trains on pairs mixed when the corpus was written).  Row b of
 * the batch is a clean window and a noise window gathered from two flat float32 arrays resident in HBM and mixed at a drawn SNR:
 *   c[j] = clean_flat[cs + j], j < length; cs clamped into [0, clean_total - length] as in wunet_crop_windows.
 *   n[j] = noise_flat[ns + (ph + j) mod nl]: the noise item [ns, ns + nl) read circularly from phase ph, so an item shorter than the
 *     window wraps as often as needed.  The item range is cut to its part inside [0, noise_total) and ph is reduced modulo the
 *     length that is left; fewer than 1 sample left (nl = 0 is how a caller asks for a clean row): no noise, g = 0.
 *   Pc = sum c^2, Pn = sum n^2 over the window (raw sums, no mean removal), in double and in one fixed order.
 *   g = sqrt(Pc / (Pn 10^(snr_db / 10))) in double; g = 0 when Pc or Pn is below length * 1e-12 (RMS 1e-6): a silent clean or noise
 *     window passes the clean window through, never Inf or NaN.
 *   a = level; with peak_limit > 0: bound = a (max|c| + g max|n|) and a <- a peak_limit / bound when bound > peak_limit (the bound is
 *     conservative - max|c + g n| <= max|c| + g max|n| - and costs no pass over the mixed row).
 *   mixture[b][j] = a (c[j] + g n[j]), clean_out[b][j] = a c[j], gains[b] = (g, a) (gains may be NULL), with g and a rounded to
 *     float32 once before use; a row with g = 0 gets mixture == clean_out bit for bit.
 * rows: device int64 [batch][4] = clean start, noise item start, noise item length, noise phase.  params: device float32 [batch][2] =
 * snr_db, level (linear).  scratch: >= wunet_mix_scratch_bytes(batch, length) device bytes, 8-byte aligned, no memset needed.
 * mixture / clean_out receive [batch][1][length] float32 (16-byte aligned when length % 4 == 0).  batch <= 65535, length <= 2^30.
 * Two launches; everything a launch depends on is read from device memory, so a captured call follows the tables it was captured on.
 * No atomics: bit-identical run to run.  Caller-owned memory, no allocation, no synchronisation. */
size_t wunet_mix_scratch_bytes(int batch, int length);
int wunet_mix_windows(const float* clean_flat, long long clean_total, const float* noise_flat, long long noise_total,
                      const long long* rows,   /* [batch][4]: clean start, noise item start, noise item length, noise phase */
                      const float* params,     /* [batch][2]: snr_db, level (linear) */
                      float peak_limit, int batch, int length, void* scratch,
                      float* mixture, float* clean_out, float* gains /* [batch][2] or NULL */, void* stream);

/* dst[b][j] = gains[b][1] * src[b][j] over [batch][length]: the level a of a `gains` table that wunet_mix_windows wrote, applied to
 * another batch - the one float32 multiply that made clean_out, so a target scaled here equals a c bit for bit.  dst == src is
 * allowed.  16-byte aligned src / dst when length % 4 == 0.  One launch, the mix's shape limits. */
int wunet_apply_level(const float* src, const float* gains /* [batch][2] */, int batch, int length, float* dst, void* stream);

/* Reverberant speech made on the device (no reference counterpart): row b is a window of the clean array convolved with a room impulse
 * response out of a second flat float32 array - a per-row FIR as an exact fp32 MFMA GEMM (csrc/wunet_reverb.h).
 *   x[t] = clean_flat[t] for t >= is and 0 in front of it: `is` is the first sample of the window's item, what lies before belongs to
 *     another utterance and does not leak in.
 *   reverberant[b][j] = sum over k < K of h[k] x[cs + j - k],  direct[b][j] = the same sum over k < min(early_taps, K), j < length.
 *   With a response that starts at its direct path with h[0] = 1 (pack_rir_shard), early_taps = 1 gives the dry window itself and
 *   early_taps at 50 ms the early-reflections target.
 * Clamps: cs into [0, clean_total - length], is into [0, cs]; the RIR range [hs, hs + K) is cut to its part inside [0, rir_total) and K
 * then to WUNET_REVERB_MAX_TAPS.  Nothing outside either array is addressed, and the loads are masked, not multiplied by zero.
 * A row with K <= 0 is passed through: both outputs are the window's own bits.  Products are exact fp32 and an output is one chain of
 * fewer than K + 256 fused adds in a fixed order: |out - exact| <= gamma(K + 256) sum |h[k]| |x[cs + j - k]|.
 * rows: device int64 [batch][4] = window start cs, item start is, RIR start hs, RIR taps K.  early_taps >= 1 is used only when direct
 * is not NULL.  reverberant / direct receive [batch][1][length] float32 (16-byte aligned when length % 4 == 0).  batch <= 65535,
 * length <= 2^30.  One launch; everything it depends on is read from device memory, so a captured launch follows its tables.  No
 * atomics: bit-identical run to run.  Caller-owned memory, no allocation, no synchronisation. */
#define WUNET_REVERB_MAX_TAPS 16384
int wunet_reverb_windows(const float* clean_flat, long long clean_total, const float* rir_flat, long long rir_total,
                         const long long* rows,   /* [batch][4]: window start, clean item start, RIR start, RIR taps */
                         int early_taps, int batch, int length,
                         float* reverberant, float* direct /* [batch][1][length] or NULL */, void* stream);

/* Chunked enhancement with overlap (the reference cuts a recording into disjoint chunks, enhancement.py:57-69; this is the same with
 * a margin dropped at every chunk edge and a cross-fade between neighbours; csrc/wunet_chunks.h).  L = length, m = margin, f = fade,
 * hop H = L - 2 m - f with H >= 1 and f <= H, so at most two chunks cover a sample.  A recording of T samples has
 * n = max(1, ceil((T - f) / H)) chunks; chunk k reads samples [k H - m, k H - m + L) of it, zeros outside [0, T), and is trusted on
 * [k H, k H + H + f).  For the output sample t < T, with k = min(t / H, n - 1), j = t - k H and y_k the model's output for chunk k:
 *   k >= 1 and j < f:  out[t] = ramp[j] y_k[m + j] + (1 - ramp[j]) y_(k-1)[m + H + j]   (1 - ramp[j] in float32, then one fma)
 *   otherwise:         out[t] = y_k[m + j], the same bits.
 * The recordings of a call lie in one flat float32 array of `total` samples, each at its own start; the output array has the same layout.
 *
 * wunet_chunk_gather: chunks[i][0][j] = flat[start + s + j] where 0 <= s + j < T and 0 <= start + s + j < total, else 0, for rows[i] =
 *   (flat start of the recording, T, chunk start s = k H - m).  Loads are masked, nothing outside `flat` is addressed.
 * wunet_chunk_overlap_add: the formula above for every recording recs[r] = (flat start, T, first chunk row, chunk count), written to
 *   out_flat[start + t].  ramp: device float32 [fade] (the window's shape is data), NULL exactly when fade == 0.  max_len: the largest
 *   T, it sizes the grid (samples beyond it are not written).  A chunk row outside [0, n), an offset outside a chunk and an output
 *   index outside [0, total) are skipped, never addressed.
 * rows / recs: device int64.  n, n_recs < 2^31, length <= 2^30.  One launch each; everything ragged is read from device memory, so a
 * captured call follows its tables.  No atomics: bit-identical run to run.  Caller-owned memory, no allocation, no synchronisation.
 * 16-byte accesses are used wherever the addresses involved are aligned, dwords elsewhere: no alignment is required. */
int wunet_chunk_gather(const float* flat, long long total, const long long* rows /* [n][3]: flat start, T, chunk start */,
                       long long n, int length, float* chunks /* [n][1][length] */, void* stream);
int wunet_chunk_overlap_add(const float* chunks /* [n][1][length] */, long long n, int length, int margin, int fade,
                            const float* ramp /* [fade] or NULL */, const long long* recs /* [n_recs][4]: flat start, T, first row, count */,
                            long long n_recs, long long max_len, float* out_flat, long long total, void* stream);

/* Rational resampling of ragged rows (no reference counterpart in code: a reference user resamples with librosa on the host;
 * csrc/wunet_resample.h): a polyphase FIR filter over many rows of different lengths that share one rate pair, one launch.
 * up / down in lowest terms; taps: device float32 h'[0 .. n_taps), n_taps = 2 L + 1, the gain `up` already folded in - the filter's
 * shape and gain are data.  For the row rows[i] = (in start, T_in, out start, T_out) and the output sample m < T_out:
 *   c = m down + L,  phase = c mod up,  i_hi = c / up
 *   out[out start + m] = sum_j h'[phase + up j] in[in start + i_hi - j]   over the j with phase + up j < n_taps and 0 <= i_hi - j < T_in
 * (zeros outside the row).  With T_out = ceil(T_in up / down) this is scipy.signal.resample_poly(x, up, down, window = h) for h' = up h;
 * a smaller T_out truncates, a larger one reads zeros behind the row.  float32 operands, products exact in double, the sum in double
 * in increasing j, one rounding to float32.  No atomics: bit-identical run to run.
 * max_out: the largest T_out, it sizes the grid (outputs beyond it are not computed).  A row whose start, length or extent lies
 * outside [0, in_total] / [0, out_total], or with a negative value, is skipped, never addressed.  rows: device int64; everything ragged
 * is read from device memory, so a captured call follows its table.  Caller-owned memory, no allocation, no synchronisation, no
 * alignment required.  -1 with wunet_last_error() text for: a null pointer; n, max_out, up or down < 1; up and down not coprime;
 * n_taps even or above WUNET_RESAMPLE_MAX_TAPS (max(up, down) above WUNET_RESAMPLE_MAX_RATIO); n >= 2^31; an array of 2^50 samples.
 * wunet_resample_tile: the outputs a block of the kernel owns per trip for that filter (what the tests put row lengths next to), 0
 *   for a filter the entry refuses. */
#define WUNET_RESAMPLE_MAX_TAPS 12801
#define WUNET_RESAMPLE_MAX_RATIO 640
int wunet_resample_rows(const float* in, long long in_total,
                        const long long* rows /* [n][4]: in start, T_in, out start, T_out */, long long n,
                        long long max_out, int up, int down, const float* taps, int n_taps,
                        float* out, long long out_total, void* stream);
long long wunet_resample_tile(int up, int down, int n_taps);

/* Cascades of second-order IIR sections over a batch of windows (no reference counterpart in code: a reference user filters on the host
 * with scipy.signal.sosfilt; csrc/wunet_sos.h): equalisers, DC blockers, pre-emphasis, band limits - everything recursive, which the FIR
 * kernels above cannot express.  One launch, one block per row.
 * Source of row b, rows[b] = (window start ws, item start is, circular length nl, phase ph), all in samples of `flat`:
 *   linear   (nl <= 0)  x[j] = flat[ws + j] where ws + j >= is, and 0 in front of the item.  ws is clamped into [0, total - length] and
 *                       is into [0, ws]; nl and ph are ignored.
 *   circular (nl >= 1)  x[j] = flat[is + ((ph + j) mod nl)], the non-negative modulo (j < 0 wraps backwards).  The item [is, is + nl) is
 *                       cut to its part inside [0, total) and ph reduced modulo what is left, as the mix entry does with a noise item; if
 *                       nothing is left the output row is zeros.  ws is ignored.
 * Lead-in: the filter starts from rest at j = -lead_b and the outputs at j < 0 are dropped, so a window cut out of the middle of a
 *   recording carries no start-up transient.  lead_b = min(lead, ws - is) for a linear row (never in front of the item), lead for a
 *   circular one.
 * Filter: `sections` sections in cascade, coefs[b][s] = (b0, b1, b2, a1, a2) with a0 = 1, each the transposed direct form II recurrence
 *   of scipy.signal.sosfilt:  o = b0 v + s0;  s0 = b1 v - a1 o + s1;  s1 = b2 v - a2 o.  The float32 coefficients are taken as exact
 *   values; all state and arithmetic are double; each output is rounded to float32 once.  out[b][0][j] for 0 <= j < length.
 *   The kernel runs the recurrence in parallel along the row, in chunks whose entry states come from a scan with the chunk's exact
 *   transition matrix; the result differs from the sequential double recurrence by double rounding only (tests/sos_cases.py).
 * Nothing outside `flat` or `out` is ever addressed, whatever the tables hold; loads are masked, not multiplied by zero.  A row whose
 * coefficients are non-finite or unstable yields an unspecified row of its own and leaves every other row's bits alone.
 * rows: device int64, coefs: device float32; everything ragged is read from device memory, so a captured call follows its tables.  No
 * atomics: bit-identical run to run.  Caller-owned memory, no allocation, no synchronisation, no alignment required.
 * -1 with the error text for: a null pointer; batch or length < 1; batch > 65535; length > 2^24; sections outside
 * [1, WUNET_SOS_MAX_SECTIONS]; lead outside [0, WUNET_SOS_MAX_LEAD]; total < length.
 * wunet_sos_tile: tile * 65536 + chunk for that count of sections - `tile` the samples (lead-in included) a block owns per trip, `chunk`
 *   (the low 16 bits) the consecutive samples one thread owns: what the tests put row lengths next to; 0 for a refused count. */
#define WUNET_SOS_MAX_SECTIONS 8
#define WUNET_SOS_MAX_LEAD 8192
int wunet_sos_windows(const float* flat, long long total,
                      const long long* rows /* [batch][4]: window start, item start, circular length, phase */,
                      const float* coefs /* [batch][sections][5]: b0 b1 b2 a1 a2 */,
                      int sections, int lead, int batch, int length, float* out /* [batch][1][length] */, void* stream);
long long wunet_sos_tile(int sections);

/* BSS Eval SDR per row (no reference counterpart in code: Wave-U-Net results are reported in it, computed on the host by
 * mir_eval.separation.bss_eval_sources / museval; csrc/wunet_bss.h): that function for ONE source - the reference padded with
 * filter_length - 1 zeros, so e_interf = 0 and SDR = SAR; no mean removal, no regularisation.  Per row, with s = clean, e = estimate,
 * both zero outside [0, len), n = filter_length:
 *   r[k] = sum_t s[t] s[t + k],  b[k] = sum_t s[t] e[t + k]  (k = 0 .. n - 1),  E = sum e^2,  G = toeplitz(r);  G c = b;
 *   P = c'b,  R = E - 2 c'b + c'G c,  out_db = 10 log10(P / R)
 * R is the residual energy of the c that was found, second order in the solver's error.  Unlike SI-SDR the score forgives the
 * estimate any n-tap filtering (colouring, delay < n) of the reference; n = 1 is SI-SDR without mean removal.
 * Two launches: correlation partials per (row, segment of wunet_bss_sdr_tile samples) - float x float products are exact in double,
 * the sums are double - then one block per row adds them in segment order, runs Levinson's recursion in double (n dependent orders,
 * the latency of the call) and rounds the score to float32 once.  No atomics: bit-identical run to run.
 * A row whose clean or estimate is all zero inside its length, or whose length is 0, yields NaN in that row (mir_eval raises there)
 * and leaves every other row's bits alone; nothing is read back.  estimate == clean bit for bit yields +inf (R = 0 exactly).
 * lengths: NULL (every row has row_len samples) or device int64 [rows], read on the device and clamped to [0, row_len], so a captured
 * call follows it; samples beyond a row's length are never addressed as data (masked loads).
 * scratch: wunet_bss_sdr_scratch_bytes(rows, row_len, filter_length) bytes, 8-byte aligned; the waveforms need 4-byte alignment only.
 * Caller-owned memory, no allocation, no synchronisation, capturable.
 * -1 with the error text for: a null pointer (lengths excepted); filter_length outside [1, WUNET_BSS_MAX_FILTER]; rows or row_len 0;
 * rows > 65535; row_len >= 2^31.  wunet_bss_sdr_scratch_bytes answers 0 for the same shapes.
 * wunet_bss_sdr_tile: the samples of a row one block of the first launch owns - what the tests put row lengths next to; 0 for a
 * refused filter_length. */
#define WUNET_BSS_MAX_FILTER 512
size_t wunet_bss_sdr_scratch_bytes(size_t rows, size_t row_len, int filter_length);
int wunet_bss_sdr_forward(const float* clean, const float* estimate, size_t rows, size_t row_len,
                          const long long* lengths /* NULL or device [rows] */, int filter_length,
                          void* scratch, float* out_db /* [rows] */, void* stream);
long long wunet_bss_sdr_tile(int filter_length);

/* Measurement aid (tools/conv_trace.py; no reference counterpart): a device buffer of gridDim.x * 64 uint64 that the DMA-staged
 * conv / data-gradient kernel (conv_h3d_kernel) fills with shader-clock stamps of each block's phases (entry; per K stage: tile
 * landed, W buffer released, MFMAs issued; epilogue done), or NULL (default) to turn the stamps off.  Process-wide. */
void wunet_debug_set_conv_trace(void* dev_buffer);

/* Single-op entry points (parity tests of the MFMA kernels against F.conv1d semantics,
 * nn.Conv1d stride 1, padding K/2, K in {5, 15}).  They allocate scratch and synchronise. */
int wunet_op_conv1d(const float* x, const float* w, const float* bias, float* z,
                    int B, int Cin, int Cout, int L, int K, void* stream);
int wunet_op_conv1d_dgrad(const float* gz, const float* w, float* dx,
                          int B, int Cin, int Cout, int L, int K, void* stream);
int wunet_op_conv1d_wgrad(const float* gz, const float* x, float* dw,
                          int B, int Cin, int Cout, int L, int K, void* stream);

/* The same three ops on the fp16-split kernels (conv_h3d_kernel of csrc/wunet_h3d.h, wgrad_h3d_kernel / wgrad_h3_kernel of csrc/wunet_h3.h) with
 * the planner's tiling for the geometry and device-derived power-of-two operand scales: L >= 16, B*L >= 256, and Cin >= 16
 * for the two gradients (the network planner's own conditions).  They allocate scratch and synchronise. */
int wunet_op_conv1d_split(const float* x, const float* w, const float* bias, float* z,
                          int B, int Cin, int Cout, int L, int K, void* stream);
int wunet_op_conv1d_dgrad_split(const float* gz, const float* w, float* dx,
                                int B, int Cin, int Cout, int L, int K, void* stream);
int wunet_op_conv1d_wgrad_split(const float* gz, const float* x, float* dw,
                                int B, int Cin, int Cout, int L, int K, void* stream);

/* (tests / tools) The same three ops on the bf16 instantiations of those kernels - the arithmetic of wunet_set_h3(ctx, 3 | 4): one bf16 word per
 * operand value (round to nearest even of the scaled value), one MFMA pass, the planner's bf16 tiling and split-K plan for the geometry.  The
 * argument lists and shape conditions of the _split entry points.  The result is the conv of the bf16-rounded operands up to fp32
 * accumulation (power-of-two scales, exact products). */
int wunet_op_conv1d_bf16(const float* x, const float* w, const float* bias, float* z,
                         int B, int Cin, int Cout, int L, int K, void* stream);
int wunet_op_conv1d_dgrad_bf16(const float* gz, const float* w, float* dx,
                               int B, int Cin, int Cout, int L, int K, void* stream);
int wunet_op_conv1d_wgrad_bf16(const float* gz, const float* x, float* dw,
                               int B, int Cin, int Cout, int L, int K, void* stream);

#ifdef __cplusplus
}
#endif
#endif
