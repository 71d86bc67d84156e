"""Loss plugins, same factory convention as the reference (/root/reference/model/loss.py:3-7):
zero-argument factories returning a module called as `loss(clean, enhanced)`
(trainer/trainer.py:36 - the prediction is the second argument).

    "loss_function": {"module": "wave-u-net-for-speech-enhancement_amd.loss", "main": "mse_loss", "args": {}}

`smooth_l1_loss` (torch.nn.SmoothL1Loss semantics, beta = 1) is the loss BASELINE.json's config 3
names; the reference only mentions it in its README.

`si_sdr_loss` / `snr_loss` (no reference counterpart): the negative mean over the utterances of the batch of the scale-invariant
SDR / the SNR in dB, each row of the last dimension on its own (include/wunet_hip.h: wunet_loss_rows_*):

    "loss_function": {"module": "wave-u-net-for-speech-enhancement_amd.loss", "main": "si_sdr_loss", "args": {}}

`stft_loss` (no reference counterpart): the multi-resolution STFT loss - spectral convergence plus log-magnitude L1 at several
window sizes (include/wunet_hip.h: wunet_stft_*); `weighted_loss` sums several of the factories above, which is what a config needs
to train on a waveform term plus the spectral one:

    "loss_function": {"module": "wave-u-net-for-speech-enhancement_amd.loss", "main": "weighted_loss",
                      "args": {"terms": [["l1_loss", 1.0], ["stft_loss", 0.5, {"fft_sizes": [1024, 2048, 512]}]]}}

`stoi_loss` (no reference counterpart): minus the mean over the utterances of the batch of STOI, the score the reference picks its best
checkpoint by, exactly as `metrics.stoi` computes it (include/wunet_hip.h: wunet_stoi_loss_*); gradient with respect to `enhanced`
only, zero where a band magnitude of the estimate is exactly 0 (autograd: NaN) and for rows with fewer than 30 spectral frames.  STOI
ignores level, and phase below its 26 ms frames, so it is usually one term beside a waveform one:

    "loss_function": {"module": "wave-u-net-for-speech-enhancement_amd.loss", "main": "weighted_loss",
                      "args": {"terms": [["l1_loss", 1.0], ["stoi_loss", 0.25, {"sample_rate": 16000}]]}}

`stoi_loss(extended=True)`: minus the mean ESTOI (Jensen & Taal 2016; as a loss: Kolbaek et al. 2018), exactly as
`metrics.stoi(extended=True)` computes it (include/wunet_hip.h: wunet_estoi_loss_*).  No min(alpha Y, clip X): no kink and no clipped
items that pass nothing; a band row or a frame column of a segment whose centred norm is exactly 0 passes no gradient (autograd: NaN):

    ["stoi_loss", 0.25, {"sample_rate": 16000, "extended": true}]

`compressed_spectral_loss` (no reference counterpart): the power-law compressed spectral loss with a complex, phase-aware term (Braun &
Tashev 2021; the DNS-challenge baseline loss; include/wunet_hip.h: wunet_cspec_*) - per STFT bin (1 - complex_weight) (A_c - A_e)^2 +
complex_weight |Z_c - Z_e|^2 with A = |S|^compress and Z = S |S|^(compress - 1), averaged; gradient with respect to `enhanced` only;
below `clamp` (on the power) the compression factors are constants, so silence still gets a gradient through the complex term:

    "loss_function": {"module": "wave-u-net-for-speech-enhancement_amd.loss", "main": "weighted_loss",
                      "args": {"terms": [["l1_loss", 1.0], ["compressed_spectral_loss", 0.5, {"compress": 0.3, "complex_weight": 0.3}]]}}

`mel_loss` (no reference counterpart): the multi-scale log-mel spectrogram loss (HiFi-GAN's mel loss; the multi-scale mel loss of DAC /
EnCodec-style codecs; include/wunet_hip.h: wunet_mel_*) - per resolution the L1 distance between the log-mel spectrograms
ln max(Phi |S|^power, floor) of the two signals (log_weight) plus that between the mel spectrograms themselves (lin_weight), averaged;
Phi is `mel_filterbank` (librosa's formulas); gradient with respect to `enhanced` only:

    "loss_function": {"module": "wave-u-net-for-speech-enhancement_amd.loss", "main": "mel_loss", "args": {"sample_rate": 16000}}
    ["mel_loss", 0.5, {"fft_sizes": [512, 1024], "hop_sizes": [128, 256], "win_lengths": [512, 1024], "n_mels": [40, 80]}]
"""
import torch
import torch.nn as nn

from .engine import MEL_MAX_FILTERS, STFT_MAX_RESOLUTIONS, check_stft_resolution, check_stoi_rate, default_engine, mel_filterbank  # noqa: F401


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kind, engine, clean, enhanced):
        clean_c, enh_c = clean.detach().contiguous(), enhanced.detach().contiguous()
        ctx.kind, ctx.engine = kind, engine
        ctx.save_for_backward(clean_c, enh_c)
        return engine.loss_forward(kind, clean_c, enh_c)

    @staticmethod
    def backward(ctx, grad_loss):
        clean, enh = ctx.saved_tensors
        g = ctx.engine.loss_backward(ctx.kind, clean, enh, grad_loss)
        g_clean = -g if ctx.needs_input_grad[2] else None
        return None, None, g_clean, (g if ctx.needs_input_grad[3] else None)


class _HipLossModule(nn.Module):
    """What every loss module here shares: the engine it runs on (`_engine_override`, which tests and tools set, or the process's)."""
    _engine_override = None

    def _engine(self):
        return self._engine_override if self._engine_override is not None else default_engine()


class HipLoss(_HipLossModule):
    def __init__(self, kind):
        super().__init__()
        self.kind = kind

    def forward(self, clean, enhanced):
        return _LossFn.apply(self.kind, self._engine(), clean, enhanced)


def mse_loss():
    return HipLoss("mse")


def l1_loss():
    return HipLoss("l1")


def smooth_l1_loss():
    return HipLoss("smooth_l1")


class _EnhancedGradFn(torch.autograd.Function):
    """The losses with a gradient with respect to `enhanced` only.  `mod` (an _EnhancedGradLoss) supplies the message of the refusal,
    _loss_forward(engine, clean, enhanced) -> (loss, tensors to save) and _loss_backward(engine, shape, saved tensors, grad_loss)."""

    @staticmethod
    def forward(ctx, mod, engine, clean, enhanced):
        if clean.requires_grad:                 # (before anything runs)
            raise NotImplementedError(mod._no_clean_grad)
        clean_c, enh_c = clean.detach().contiguous(), enhanced.detach().contiguous()
        loss, saved = mod._loss_forward(engine, clean_c, enh_c)
        ctx.mod, ctx.engine, ctx.shape = mod, engine, tuple(enh_c.shape)
        ctx.save_for_backward(*saved)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        g = ctx.mod._loss_backward(ctx.engine, ctx.shape, ctx.saved_tensors, grad_loss) if ctx.needs_input_grad[3] else None
        return None, None, None, g


class _EnhancedGradLoss(_HipLossModule):
    def forward(self, clean, enhanced):
        return _EnhancedGradFn.apply(self, self._engine(), clean, enhanced)


class HipRowLoss(_EnhancedGradLoss):
    """loss(clean, enhanced) -> -mean over rows of si_sdr / snr [dB]; the last dimension is the utterance."""

    def __init__(self, kind, zero_mean=True, eps=1e-8):
        super().__init__()
        if not (eps >= 0.0 and eps < float("inf")):
            raise ValueError(f"{kind}_loss: eps must be finite and >= 0 (got {eps})")
        self.kind, self.zero_mean, self.eps = kind, bool(zero_mean), float(eps)
        self._no_clean_grad = (f"{kind}_loss: no gradient with respect to `clean` (the target also sets the signal energy, so it is "
                               "not minus the gradient of `enhanced` as for the element-wise losses): detach it")

    def _loss_forward(self, engine, clean, enhanced):
        loss, coefs, _ = engine.loss_rows_forward(self.kind, clean, enhanced, self.zero_mean, self.eps)
        return loss, (clean, enhanced, coefs)

    def _loss_backward(self, engine, shape, saved, grad_loss):
        return engine.loss_rows_backward(self.kind, *saved, grad_loss)


def si_sdr_loss(zero_mean=True, eps=1e-8):
    return HipRowLoss("si_sdr", zero_mean, eps)


def snr_loss(zero_mean=True, eps=1e-8):
    return HipRowLoss("snr", zero_mean, eps)


def _check_resolutions(name, fft_sizes, hop_sizes, win_lengths):
    """The three lists of a spectral loss, zipped into (n_fft, hop, win_length) triples for check_stft_resolution."""
    fft_sizes, hop_sizes, win_lengths = list(fft_sizes), list(hop_sizes), list(win_lengths)
    if not (len(fft_sizes) == len(hop_sizes) == len(win_lengths)):
        raise ValueError(f"{name}: fft_sizes, hop_sizes and win_lengths must have equal lengths (got {len(fft_sizes)}, "
                         f"{len(hop_sizes)}, {len(win_lengths)})")
    if not 1 <= len(fft_sizes) <= STFT_MAX_RESOLUTIONS:
        raise ValueError(f"{name}: 1 .. {STFT_MAX_RESOLUTIONS} resolutions (got {len(fft_sizes)})")
    return list(zip(fft_sizes, hop_sizes, win_lengths))


class HipStftLoss(_EnhancedGradLoss):
    """loss(clean, enhanced) -> mean over the resolutions of sc_weight * spectral convergence + mag_weight * log-magnitude L1; the last
    dimension is the utterance.  Gradient with respect to `enhanced` only."""
    _no_clean_grad = ("stft_loss: no gradient with respect to `clean` (the target also sets the spectral-convergence "
                      "norm, so it is not minus the gradient of `enhanced`): detach it")

    def __init__(self, fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50), win_lengths=(600, 1200, 240), sc_weight=1.0, mag_weight=1.0,
                 clamp=1e-7):
        super().__init__()
        triples = _check_resolutions("stft_loss", fft_sizes, hop_sizes, win_lengths)
        if not (clamp > 0.0 and clamp < float("inf")):
            raise ValueError(f"stft_loss: clamp must be finite and > 0 (got {clamp})")
        self.resolutions = tuple(check_stft_resolution(n, h, w) for n, h, w in triples)
        self.sc_weight, self.mag_weight, self.clamp = float(sc_weight), float(mag_weight), float(clamp)

    def _loss_forward(self, engine, clean, enhanced):
        loss, coefs, saved = engine.stft_loss_forward(clean, enhanced, self.resolutions, self.sc_weight, self.mag_weight, self.clamp)
        return loss, (coefs, *saved)

    def _loss_backward(self, engine, shape, saved, grad_loss):
        return engine.stft_loss_backward(shape, self.resolutions, saved[0], list(saved[1:]), grad_loss, self.clamp)


def stft_loss(fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50), win_lengths=(600, 1200, 240), sc_weight=1.0, mag_weight=1.0, clamp=1e-7):
    return HipStftLoss(fft_sizes, hop_sizes, win_lengths, sc_weight, mag_weight, clamp)


class HipCompressedSpectralLoss(_EnhancedGradLoss):
    """loss(clean, enhanced) -> mean over the resolutions of mean [(1 - complex_weight) (A_c - A_e)^2 + complex_weight |Z_c - Z_e|^2]
    with A = max(P, clamp)^(compress / 2), Z = (re + i im) max(P, clamp)^((compress - 1) / 2), P = re^2 + im^2 of the STFT (stft_loss's
    conventions); the last dimension is the utterance.  Gradient with respect to `enhanced` only."""
    _no_clean_grad = "compressed_spectral_loss: no gradient with respect to `clean`: detach it"

    def __init__(self, fft_sizes=(512,), hop_sizes=(128,), win_lengths=(512,), compress=0.3, complex_weight=0.3, clamp=1e-7):
        super().__init__()
        name = "compressed_spectral_loss"
        triples = _check_resolutions(name, fft_sizes, hop_sizes, win_lengths)
        if not (compress > 0.0 and compress <= 1.0):
            raise ValueError(f"{name}: compress must be in (0, 1] (got {compress})")
        if not (complex_weight >= 0.0 and complex_weight <= 1.0):
            raise ValueError(f"{name}: complex_weight must be in [0, 1] (got {complex_weight})")
        if not (clamp > 0.0 and clamp < float("inf")):
            raise ValueError(f"{name}: clamp must be finite and > 0 (got {clamp})")
        self.resolutions = tuple(check_stft_resolution(n, h, w) for n, h, w in triples)
        self.compress, self.complex_weight, self.clamp = float(compress), float(complex_weight), float(clamp)

    def _loss_forward(self, engine, clean, enhanced):
        loss, coefs, saved = engine.cspec_loss_forward(clean, enhanced, self.resolutions, self.compress, self.complex_weight, self.clamp)
        return loss, (coefs, *saved)

    def _loss_backward(self, engine, shape, saved, grad_loss):
        return engine.cspec_loss_backward(shape, self.resolutions, saved[0], list(saved[1:]), grad_loss, self.compress, self.clamp)


def compressed_spectral_loss(fft_sizes=(512,), hop_sizes=(128,), win_lengths=(512,), compress=0.3, complex_weight=0.3, clamp=1e-7):
    return HipCompressedSpectralLoss(fft_sizes, hop_sizes, win_lengths, compress, complex_weight, clamp)


class HipMelLoss(_EnhancedGradLoss):
    """loss(clean, enhanced) -> mean over the resolutions of mean [log_weight |ln max(m_c, floor) - ln max(m_e, floor)| + lin_weight
    |m_c - m_e|] with m = Phi max(P, clamp)^(power / 2), P = re^2 + im^2 of the STFT (stft_loss's conventions) and Phi the
    `mel_filterbank` of (sample_rate, n_fft, n_mels[i], fmin, fmax, mel_scale, norm); the last dimension is the utterance.  Gradient with
    respect to `enhanced` only.  The first call on a device uploads the filterbanks: capture a step graph after one eager call, as for
    stft_loss."""
    _no_clean_grad = "mel_loss: no gradient with respect to `clean`: detach it"

    def __init__(self, sample_rate=16000, fft_sizes=(512, 1024, 2048), hop_sizes=(128, 256, 512), win_lengths=(512, 1024, 2048),
                 n_mels=(40, 80, 128), fmin=0.0, fmax=None, mel_scale="slaney", norm="slaney", power=1.0, log_weight=1.0, lin_weight=0.0,
                 clamp=1e-7, floor=1e-5):
        super().__init__()
        name = "mel_loss"
        triples = _check_resolutions(name, fft_sizes, hop_sizes, win_lengths)
        n_mels = [n_mels] * len(triples) if isinstance(n_mels, int) else list(n_mels)
        if len(n_mels) != len(triples):
            raise ValueError(f"{name}: n_mels must be one int or one per resolution (got {len(n_mels)} for {len(triples)} resolutions)")
        if any(int(n) != n or n < 1 or n > MEL_MAX_FILTERS for n in n_mels):
            raise ValueError(f"{name}: n_mels must be integers in 1 .. {MEL_MAX_FILTERS} (got {n_mels})")
        if power not in (1, 2):
            raise ValueError(f"{name}: power must be 1 or 2 (got {power})")
        for what, v in (("log_weight", log_weight), ("lin_weight", lin_weight)):
            if not (v >= 0.0 and v < float("inf")):
                raise ValueError(f"{name}: {what} must be finite and >= 0 (got {v})")
        if log_weight == 0.0 and lin_weight == 0.0:
            raise ValueError(f"{name}: log_weight and lin_weight must not both be 0")
        for what, v in (("clamp", clamp), ("floor", floor)):
            if not (v > 0.0 and v < float("inf")):
                raise ValueError(f"{name}: {what} must be finite and > 0 (got {v})")
        self.resolutions = tuple(check_stft_resolution(n, h, w) for n, h, w in triples)
        self.n_mels = tuple(int(n) for n in n_mels)
        self.sample_rate, self.fmin, self.fmax, self.mel_scale, self.norm = float(sample_rate), float(fmin), fmax, mel_scale, norm
        for (n, _, _), nm in zip(self.resolutions, self.n_mels):          # (every ValueError of the bank now, before anything runs)
            mel_filterbank(self.sample_rate, n, nm, self.fmin, self.fmax, mel_scale, norm)
        self.power, self.log_weight, self.lin_weight = int(power), float(log_weight), float(lin_weight)
        self.clamp, self.floor = float(clamp), float(floor)

    def _banks(self, engine, device):
        return [engine.mel_bank(device, self.sample_rate, n, nm, self.fmin, self.fmax, self.mel_scale, self.norm)
                for (n, _, _), nm in zip(self.resolutions, self.n_mels)]

    def _loss_forward(self, engine, clean, enhanced):
        loss, coefs, saved = engine.mel_loss_forward(clean, enhanced, self.resolutions, self._banks(engine, enhanced.device), self.power,
                                                     self.log_weight, self.lin_weight, self.clamp, self.floor)
        return loss, (coefs, *saved)

    def _loss_backward(self, engine, shape, saved, grad_loss):
        return engine.mel_loss_backward(shape, self.resolutions, self._banks(engine, saved[0].device), saved[0], list(saved[1:]), grad_loss,
                                        self.power, self.clamp, self.floor)


def mel_loss(sample_rate=16000, fft_sizes=(512, 1024, 2048), hop_sizes=(128, 256, 512), win_lengths=(512, 1024, 2048), n_mels=(40, 80, 128),
             fmin=0.0, fmax=None, mel_scale="slaney", norm="slaney", power=1.0, log_weight=1.0, lin_weight=0.0, clamp=1e-7, floor=1e-5):
    return HipMelLoss(sample_rate, fft_sizes, hop_sizes, win_lengths, n_mels, fmin, fmax, mel_scale, norm, power, log_weight, lin_weight,
                      clamp, floor)


class HipStoiLoss(_EnhancedGradLoss):
    """loss(clean, enhanced) -> -mean over rows of STOI (pystoi, extended=False; ESTOI with extended=True) at `sample_rate`; the last
    dimension is the utterance.  Gradient with respect to `enhanced` only.  The first call on a device builds the rate's tables (shared
    by both modes): capture a step graph after one eager call, as for stft_loss."""
    _no_clean_grad = ("stoi_loss: no gradient with respect to `clean` (the target also sets the silent-frame mask and "
                      "the clipping level, so it is not minus the gradient of `enhanced`): detach it")

    def __init__(self, sample_rate=16000, extended=False):
        super().__init__()
        self.sample_rate = check_stoi_rate(sample_rate)
        self.extended = bool(extended)

    def _loss_forward(self, engine, clean, enhanced):
        loss, saved, _ = engine.stoi_loss_forward(clean, enhanced, self.sample_rate, extended=self.extended)
        return loss, (saved,)

    def _loss_backward(self, engine, shape, saved, grad_loss):
        return engine.stoi_loss_backward(shape, saved[0], grad_loss, self.sample_rate, extended=self.extended)


def stoi_loss(sample_rate=16000, extended=False):
    return HipStoiLoss(sample_rate, extended)


class WeightedLoss(nn.Module):
    """The weighted sum of several of this module's losses: terms = [[factory_name, weight, args?], ...]; plain autograd over the
    terms' own functions."""

    def __init__(self, terms):
        super().__init__()
        if not terms:
            raise ValueError("weighted_loss: at least one term")
        mods, weights = [], []
        for term in terms:
            if len(term) not in (2, 3):
                raise ValueError(f"weighted_loss: a term is [factory_name, weight] or [factory_name, weight, args] (got {term!r})")
            name, weight = term[0], float(term[1])
            factory = globals().get(name)
            if name not in _FACTORIES + _SPECTRAL_FACTORIES or factory is None:
                raise ValueError(f"weighted_loss: unknown loss {name!r} (one of {sorted(_FACTORIES + _SPECTRAL_FACTORIES)})")
            mods.append(factory(**(dict(term[2]) if len(term) == 3 else {})))
            weights.append(weight)
        self.terms = nn.ModuleList(mods)
        self.weights = weights

    def forward(self, clean, enhanced):
        total = None
        for w, m in zip(self.weights, self.terms):
            v = w * m(clean, enhanced)
            total = v if total is None else total + v
        return total


_FACTORIES = ("mse_loss", "l1_loss", "smooth_l1_loss", "si_sdr_loss", "snr_loss", "stft_loss", "stoi_loss")
_SPECTRAL_FACTORIES = ("compressed_spectral_loss", "mel_loss")       # the factories added since: WeightedLoss consults both tuples


def weighted_loss(terms):
    return WeightedLoss(terms)
