"""Scores computed on the device.  The reference's validation epoch scores STOI and PESQ on the host, per recording
(trainer/trainer.py:58-143): `stoi` below is that STOI (pystoi, extended=False) as HIP kernels; PESQ (ITU-T P.862, a long procedural
model) stays a host metric and out of scope - SURVEY.md §2.  `si_sdr` / `snr` are the forward of the row losses (include/wunet_hip.h:
wunet_loss_rows_forward) with its per-row output: one pass over the pair, sums in double, no backward; float32 [rows] in dB.
`sdr` is the BSS Eval SDR the Wave-U-Net literature reports (mir_eval.separation.bss_eval_sources for one source; include/wunet_hip.h:
wunet_bss_sdr_forward).  The scores available on the device are therefore SI-SDR, SNR, BSS Eval SDR, STOI and ESTOI.
The last dimension is the utterance; all leading dimensions are flattened to rows.  Results live on the inputs' device.
"""
import torch

from .engine import default_engine


@torch.no_grad()
def _rows(kind, clean, estimate, zero_mean, eps, engine):
    engine = engine if engine is not None else default_engine()
    _, _, rows = engine.loss_rows_forward(kind, clean.detach().contiguous(), estimate.detach().contiguous(), zero_mean, eps,
                                          per_row=True, with_backward=False)
    return rows


def si_sdr(clean, estimate, zero_mean=True, eps=1e-8, engine=None):
    """Scale-invariant SDR of `estimate` against `clean`, per row."""
    return _rows("si_sdr", clean, estimate, zero_mean, eps, engine)


def snr(clean, estimate, zero_mean=True, eps=1e-8, engine=None):
    """SNR of `estimate` against `clean`, per row."""
    return _rows("snr", clean, estimate, zero_mean, eps, engine)


def si_sdr_improvement(clean, noisy, enhanced, zero_mean=True, eps=1e-8, engine=None):
    """SI-SDR of the enhanced signal minus SI-SDR of the noisy one, per row: what the enhancement gained."""
    return si_sdr(clean, enhanced, zero_mean, eps, engine) - si_sdr(clean, noisy, zero_mean, eps, engine)


@torch.no_grad()
def sdr(clean, estimate, filter_length=512, lengths=None, engine=None):
    """BSS Eval SDR of `estimate` against `clean`, per row, in dB: mir_eval.separation.bss_eval_sources(clean[None], estimate[None])
    for one source - the energy of the projection of the estimate onto the reference and its delays 0 .. filter_length - 1 over the
    energy of the rest; no mean removal.  Unlike SI-SDR it forgives a filter of up to filter_length (1 .. 512) taps; filter_length=1
    is si_sdr(zero_mean=False, eps=0).  lengths: None, or int64 [rows] on the device - row i counts as its first lengths[i] samples
    (ragged recordings in one padded slab).  A row whose reference or estimate is silent, or of length 0, scores NaN (mir_eval raises
    there; nothing is read back here), estimate == clean scores +inf.  Returns float32 [rows]."""
    engine = engine if engine is not None else default_engine()
    return engine.bss_sdr(clean.detach().contiguous(), estimate.detach().contiguous(), filter_length, lengths)


def sdr_improvement(clean, noisy, enhanced, filter_length=512, lengths=None, engine=None):
    """BSS Eval SDR of the enhanced signal minus that of the noisy one, per row: what the enhancement gained."""
    return sdr(clean, enhanced, filter_length, lengths, engine) - sdr(clean, noisy, filter_length, lengths, engine)


@torch.no_grad()
def stft_magnitude(x, n_fft=320, hop=160, win_length=320, engine=None):
    """|STFT| of every row of x on the device - the spectrum the reference's validation epoch looks at on the host
    (trainer/trainer.py:108-110: n_fft 320, hop 160), torch.stft's conventions (periodic Hann, center=True, reflect padding).  The
    forward GEMM of the STFT loss with its magnitude output only (include/wunet_hip.h: wunet_stft_forward), no clamp.
    Returns float32 [rows, 1 + T // hop, n_fft // 2 + 1]."""
    engine = engine if engine is not None else default_engine()
    return engine.stft_magnitude(x.detach().contiguous(), n_fft, hop, win_length)


@torch.no_grad()
def mel_spectrogram(x, sample_rate=16000, n_fft=512, hop=128, win_length=512, n_mels=80, fmin=0.0, fmax=None, mel_scale="slaney",
                    norm="slaney", power=1.0, log=False, floor=1e-5, engine=None):
    """The mel spectrogram of every row of x on the device: m = Phi |STFT|^power with stft_magnitude's conventions (no clamp) and Phi
    the `loss.mel_filterbank` of (sample_rate, n_fft, n_mels, fmin, fmax, mel_scale, norm) - the forward of `loss.mel_loss` for one
    signal (include/wunet_hip.h: wunet_mel_forward without `clean`).  log=True: ln max(m, floor), natural log.
    Returns float32 [rows, 1 + T // hop, n_mels]."""
    if power not in (1, 2):
        raise ValueError(f"mel_spectrogram: power must be 1 or 2 (got {power})")
    if log and not (floor > 0.0 and floor < float("inf")):
        raise ValueError(f"mel_spectrogram: floor must be finite and > 0 (got {floor})")
    engine = engine if engine is not None else default_engine()
    bank = engine.mel_bank(x.device, sample_rate, n_fft, n_mels, fmin, fmax, mel_scale, norm)
    return engine.mel_spectrogram(x.detach().contiguous(), bank, n_fft, hop, win_length, int(power), float(floor) if log else 0.0)


@torch.no_grad()
def stoi(clean, estimate, sample_rate=16000, return_frames=False, engine=None, extended=False):
    """Short-time objective intelligibility of `estimate` against `clean`, per row: Taal et al. 2011 as pystoi computes it for
    stoi(clean, estimate, sample_rate, extended=False) - what the reference's validation epoch calls on the host at 16 kHz
    (util/utils.py:116-117) - on the device (include/wunet_hip.h: wunet_stoi_forward), without a host read: a row with fewer than 30
    spectral frames after the removal of its silent frames scores 1e-5 (pystoi's value; its warning is not reproduced).
    Returns float32 [rows]; with return_frames also int32 [rows], the spectral frame count of every row.  The tables of a
    (device, sample_rate) are built on the first call; later calls allocate from torch's caching allocator only and can be captured.
    extended=True: ESTOI (Jensen & Taal 2016), the other branch of the same pystoi call (include/wunet_hip.h: wunet_estoi_forward) - the
    same resampler, silent-frame removal, spectra, frame counts and tables; every segment's 30 x 15 block of band magnitudes is
    normalised per band and then per frame instead of clipped.  pystoi's EPS * randn dither before each normalisation is not added:
    EPS stands in the denominators, a difference at the 1e-15 level."""
    engine = engine if engine is not None else default_engine()
    return engine.stoi(clean.detach().contiguous(), estimate.detach().contiguous(), sample_rate, return_frames, extended=bool(extended))
