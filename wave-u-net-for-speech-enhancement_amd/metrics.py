"""Scores computed on the device (no reference counterpart: the reference's validation epoch scores STOI / PESQ on the host,
trainer/trainer.py:58-108, which stay out of scope - SURVEY.md §2).  Each call is the forward of the row losses
(include/wunet_hip.h: wunet_loss_rows_forward) with its per-row output: one pass over the pair, sums in double, no backward.
The last dimension is the utterance; all leading dimensions are flattened to rows.  Returns float32 [rows] in dB on the inputs' device.
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
def stft_magnitude(x, n_fft=320, hop=160, win_length=320, engine=None):
    """|STFT| of every row of x on the device - the spectrum the reference's validation epoch looks at on the host
    (trainer/trainer.py:108-110: n_fft 320, hop 160), torch.stft's conventions (periodic Hann, center=True, reflect padding).  The
    forward GEMM of the STFT loss with its magnitude output only (include/wunet_hip.h: wunet_stft_forward), no clamp.
    Returns float32 [rows, 1 + T // hop, n_fft // 2 + 1]."""
    engine = engine if engine is not None else default_engine()
    return engine.stft_magnitude(x.detach().contiguous(), n_fft, hop, win_length)
