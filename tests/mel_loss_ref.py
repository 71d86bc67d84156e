"""Yardsticks of the mel loss tests (tests/test_mel_loss_emu.py, tests/test_gpu_mel_loss.py).  No test functions.
Three computations of the same loss, all on the CPU, as in tests/cspec_loss_ref.py (whose spectra, and tests/stft_loss_ref.py's inputs and
distances, are reused):
  (i)   oracle64    the definition in float64: torch.stft(center=True, pad_mode="reflect", return_complex=True) and this file's own
                    float64 restatement of the filterbank formulas (filterbank64), under autograd;
  (ii)  restate32   reflect pad, unfold, times the float32 basis with torch.matmul, times the float32 filterbank with torch.matmul;
  (iii) fft32       the oracle's own graph in float32 (torch's FFT).
The kernels are never compared with (ii) or (iii): those two only say how far float32 arithmetic lands from (i) on the same inputs,
d_ref = max(d(ii), d(iii)), and the kernels' bars are multiples of d_ref (bars() below).

The definition, per resolution, with Phi [n_mels, bins]:
    P = re^2 + im^2,  Pc = clamp(P, min=clamp),  S = Pc^(power / 2),  m = S Phi^T,  l = ln clamp(m, min=floor)
    L_i = mean [log_weight |l_c - l_e| + lin_weight |m_c - m_e|],  loss = mean over the resolutions of L_i.
Phi: n_mels + 2 points equally spaced in mel between mel(fmin) and mel(fmax), back in Hz p; triangle j rises over p[j] .. p[j+1] and
falls over p[j+1] .. p[j+2] at the bin frequencies b sample_rate / n_fft; norm "slaney": times 2 / (p[j+2] - p[j])."""
import functools
import math

import torch

from cspec_loss_ref import spec_fft, spec_matmul
from stft_loss_ref import CLAMP, d_loss, d_max, pair  # noqa: F401  (pair: the cases' inputs)

FLOOR = 1e-5
DEFAULTS = dict(sample_rate=16000, fmin=0.0, fmax=None, mel_scale="slaney", norm="slaney", power=1, log_weight=1.0, lin_weight=0.0,
                clamp=CLAMP, floor=FLOOR)


def _to_mel(f, scale):
    if scale == "htk":
        return 2595.0 * math.log10(1.0 + f / 700.0)
    return f * 3.0 / 200.0 if f < 1000.0 else 15.0 + math.log(f / 1000.0) * 27.0 / math.log(6.4)


def _to_hz(m, scale):
    if scale == "htk":
        return 700.0 * (math.pow(10.0, m / 2595.0) - 1.0)
    return m * 200.0 / 3.0 if m < 15.0 else 1000.0 * math.exp((m - 15.0) * math.log(6.4) / 27.0)


def mel_points(sample_rate, n_mels, fmin, fmax, mel_scale):
    """p[0 .. n_mels + 1] in Hz, plain Python floats."""
    fmax = sample_rate / 2.0 if fmax is None else fmax
    lo, hi = _to_mel(float(fmin), mel_scale), _to_mel(float(fmax), mel_scale)
    return [_to_hz(lo + (hi - lo) * i / (n_mels + 1), mel_scale) for i in range(n_mels + 2)]


@functools.lru_cache(maxsize=None)
def filterbank64(sample_rate, n_fft, n_mels, fmin=0.0, fmax=None, mel_scale="slaney", norm="slaney"):
    """The filterbank from the formulas, cell by cell in Python floats (float64): [n_mels, n_fft // 2 + 1]."""
    p = mel_points(sample_rate, n_mels, fmin, fmax, mel_scale)
    fb = torch.zeros(n_mels, n_fft // 2 + 1, dtype=torch.float64)
    for j in range(n_mels):
        scale = 2.0 / (p[j + 2] - p[j]) if norm == "slaney" else 1.0
        for b in range(n_fft // 2 + 1):
            f = b * float(sample_rate) / n_fft
            fb[j, b] = max(0.0, min((f - p[j]) / (p[j + 1] - p[j]), (p[j + 2] - f) / (p[j + 2] - p[j + 1]))) * scale
    return fb


def mel_of(spec, x, res, fb, power, clamp):
    re, im = spec(x, *res)
    pc = torch.clamp(re ** 2 + im ** 2, min=clamp) if clamp > 0.0 else re ** 2 + im ** 2
    s = pc if power == 2 else torch.sqrt(pc)
    return torch.matmul(s, fb.to(s.dtype).t())


def loss_of(spec, c, e, resolutions, n_mels, kw):
    total = 0.0
    for res, nm in zip(resolutions, n_mels):
        fb = filterbank64(kw["sample_rate"], res[0], nm, kw["fmin"], kw["fmax"], kw["mel_scale"], kw["norm"])
        m_c, m_e = (mel_of(spec, x, res, fb, kw["power"], kw["clamp"]) for x in (c, e))
        l_c, l_e = (torch.log(torch.clamp(m, min=kw["floor"])) for m in (m_c, m_e))
        total = total + (kw["log_weight"] * (l_c - l_e).abs() + kw["lin_weight"] * (m_c - m_e).abs()).mean()
    return total / len(resolutions)


def _with_grad(spec, c, e, resolutions, n_mels, kw, dtype):
    x = e.to(dtype).clone().requires_grad_(True)
    loss = loss_of(spec, c.to(dtype), x, resolutions, n_mels, kw)
    loss.backward()
    return loss.detach().double(), x.grad.double()


def knobs(**kw):
    full = dict(DEFAULTS)
    full.update(kw)
    return full


def oracle64(c, e, resolutions, n_mels, **kw):
    return _with_grad(spec_fft, c, e, resolutions, n_mels, knobs(**kw), torch.float64)


def restate32(c, e, resolutions, n_mels, **kw):
    return _with_grad(spec_matmul, c, e, resolutions, n_mels, knobs(**kw), torch.float32)


def fft32(c, e, resolutions, n_mels, **kw):
    return _with_grad(spec_fft, c, e, resolutions, n_mels, knobs(**kw), torch.float32)


@functools.lru_cache(maxsize=None)
def case_reference(rows, T, resolutions, n_mels, kw_items=()):
    """Everything the tests of one case share, computed once and left unchanged: inputs, the float64 loss and gradient, d_ref of each,
    and what the bars' conditions are asserted on: the share of bins of either signal whose float64 power lies below 10 * clamp, the
    share of cells under non-empty filters whose float64 m lies below 10 * floor, the smallest |l_c - l_e| over those cells, and the
    number of empty filters."""
    c, e = pair(rows, T)
    kw = dict(kw_items)
    full = knobs(**kw)
    l64, g64 = oracle64(c, e, resolutions, n_mels, **kw)
    l_r, g_r = restate32(c, e, resolutions, n_mels, **kw)
    l_f, g_f = fft32(c, e, resolutions, n_mels, **kw)
    low, count, low_m, cells, gap, empty = 0, 0, 0, 0, float("inf"), 0
    for res, nm in zip(resolutions, n_mels):
        fb = filterbank64(full["sample_rate"], res[0], nm, full["fmin"], full["fmax"], full["mel_scale"], full["norm"])
        live = fb.max(dim=1).values > 0.0
        empty += int((~live).sum())
        ms = []
        for x in (c, e):
            re, im = spec_fft(x.double(), *res)
            low += int((re ** 2 + im ** 2 < 10.0 * full["clamp"]).sum())
            count += re.numel()
            ms.append(mel_of(spec_fft, x.double(), res, fb, full["power"], full["clamp"])[..., live])
        for m in ms:
            low_m += int((m < 10.0 * full["floor"]).sum())
            cells += m.numel()
        l_c, l_e = (torch.log(torch.clamp(m, min=full["floor"])) for m in ms)
        gap = min(gap, float((l_c - l_e).abs().min()))
    return {"c": c, "e": e, "loss": l64, "grad": g64, "d_loss": max(d_loss(l_r, l64), d_loss(l_f, l64)),
            "d_grad": max(d_max(g_r, g64), d_max(g_f, g64)), "low_share": low / count, "low_mel_share": low_m / cells, "min_gap": gap,
            "empty": empty}


@functools.lru_cache(maxsize=None)
def spectrogram_reference(rows, T, res, n_mels, log, kw_items=()):
    """The float64 mel spectrogram of the case's `enhanced` (no clamp; ln max(m, floor) with log) and d_ref of the two float32 ones."""
    _, e = pair(rows, T)
    full = knobs(**dict(kw_items))
    fb = filterbank64(full["sample_rate"], res[0], n_mels, full["fmin"], full["fmax"], full["mel_scale"], full["norm"])

    def one(spec, x):
        m = mel_of(spec, x, res, fb, full["power"], 0.0)
        return torch.log(torch.clamp(m, min=full["floor"])) if log else m

    m64 = one(spec_fft, e.double())
    return {"e": e, "mel": m64, "d_mel": max(d_max(one(spec_matmul, e), m64), d_max(one(spec_fft, e), m64))}


def bars(ref):
    """loss: 4 d_ref + 2^-23 (the one rounding of the double result to float); gradient: 4 d_ref (max-norm relative) - the margins of
    the STFT loss, for the reason given in stft_loss_ref.bars: the kernels do the float32 work of restate32 in another order of sums."""
    return 4.0 * ref["d_loss"] + 2.0 ** -23, 4.0 * ref["d_grad"]
