"""Yardsticks and inputs of the multi-resolution STFT loss tests (tests/test_stft_loss_emu.py, tests/test_gpu_stft_loss.py).  No test
functions.  Three computations of the same loss, all on the CPU:
  (i)   oracle64    the definition in float64: torch.stft(center=True, pad_mode="reflect", return_complex=True) under autograd;
  (ii)  restate32   the kernels' algorithm restated in float32: reflect pad, unfold, times a basis computed in float64 and rounded to
                    float32, with torch.matmul;
  (iii) fft32       the oracle's own graph in float32 (torch's FFT).
The kernels are never compared with (ii) or (iii): those two only say how far float32 arithmetic lands from (i) on the same inputs,
d_ref = max(d(ii), d(iii)), and the kernels' bars are multiples of d_ref (bars() below)."""
import functools
import math

import torch

CLAMP = 1e-7


def pair(rows, T):
    """c = 0.1 randn + 0.3 sin(2 pi 0.013 t), e = c + 0.05 randn, drawn in float64 from seed 0 (per case, so that a case does not
    depend on which ran before it) and rounded to float32.  Shapes [rows, 1, T]."""
    g = torch.Generator().manual_seed(0)
    t = torch.arange(T, dtype=torch.float64)
    c = 0.1 * torch.randn(rows, 1, T, generator=g, dtype=torch.float64) + 0.3 * torch.sin(2.0 * math.pi * 0.013 * t)
    e = c + 0.05 * torch.randn(rows, 1, T, generator=g, dtype=torch.float64)
    return c.float(), e.float()


def power_fft(x, N, H, W):
    """re^2 + im^2 of torch.stft in x's dtype: [rows, F, bins]."""
    T = x.shape[-1]
    win = torch.hann_window(W, periodic=True, dtype=x.dtype)
    X = torch.stft(x.reshape(-1, T), N, hop_length=H, win_length=W, window=win, center=True, pad_mode="reflect", return_complex=True)
    return (X.real ** 2 + X.imag ** 2).transpose(1, 2)


@functools.lru_cache(maxsize=None)
def basis32(N, W):
    """The windowed DFT basis in float64, rounded once to float32: ([N, bins] cos, [N, bins] -sin)."""
    k = torch.arange(N, dtype=torch.int64)[:, None]
    b = torch.arange(N // 2 + 1, dtype=torch.int64)[None, :]
    ph = ((k * b) % N).double() * (2.0 * math.pi / N)
    w = torch.zeros(N, dtype=torch.float64)
    left = (N - W) // 2
    w[left:left + W] = torch.hann_window(W, periodic=True, dtype=torch.float64)
    return (w[:, None] * torch.cos(ph)).float(), (-w[:, None] * torch.sin(ph)).float()


def power_matmul(x, N, H, W):
    """The same spectrum as frames x basis in float32: [rows, F, bins]."""
    T = x.shape[-1]
    xp = torch.nn.functional.pad(x.reshape(-1, 1, T), (N // 2, N // 2), mode="reflect")[:, 0]
    frames = xp.unfold(-1, N, H)
    bc, bs = basis32(N, W)
    re, im = torch.matmul(frames, bc), torch.matmul(frames, bs)
    return re ** 2 + im ** 2


def loss_of(power, c, e, resolutions, sc_weight=1.0, mag_weight=1.0, clamp=CLAMP):
    total = 0.0
    for N, H, W in resolutions:
        sc_ = torch.sqrt(torch.clamp(power(c, N, H, W), min=clamp))
        se_ = torch.sqrt(torch.clamp(power(e, N, H, W), min=clamp))
        conv = torch.sqrt(((sc_ - se_) ** 2).sum()) / torch.sqrt((sc_ ** 2).sum())
        mag = (torch.log(sc_) - torch.log(se_)).abs().mean()
        total = total + sc_weight * conv + mag_weight * mag
    return total / len(resolutions)


def _with_grad(power, c, e, resolutions, dtype, **kw):
    x = e.to(dtype).clone().requires_grad_(True)
    loss = loss_of(power, c.to(dtype), x, resolutions, **kw)
    loss.backward()
    return loss.detach().double(), x.grad.double()


def oracle64(c, e, resolutions, **kw):
    return _with_grad(power_fft, c, e, resolutions, torch.float64, **kw)


def restate32(c, e, resolutions, **kw):
    return _with_grad(power_matmul, c, e, resolutions, torch.float32, **kw)


def fft32(c, e, resolutions, **kw):
    return _with_grad(power_fft, c, e, resolutions, torch.float32, **kw)


def d_loss(x, x64):
    return abs(float(x) - float(x64)) / abs(float(x64))


def d_max(x, x64):
    return ((x.double().cpu() - x64).abs().max() / x64.abs().max()).item()


@functools.lru_cache(maxsize=None)
def case_reference(rows, T, resolutions):
    """Everything the tests of one case share, computed once and left unchanged: inputs, the float64 loss and gradient, the float64
    magnitudes of e per resolution, d_ref of each, and the share of bins whose float64 power lies below 10 * clamp."""
    c, e = pair(rows, T)
    l64, g64 = oracle64(c, e, resolutions)
    l_r, g_r = restate32(c, e, resolutions)
    l_f, g_f = fft32(c, e, resolutions)
    mags, d_mag, low, count = [], [], 0, 0
    for N, H, W in resolutions:
        p64 = power_fft(e.double(), N, H, W)
        m64 = torch.sqrt(p64)
        mags.append(m64)
        d_mag.append(max(d_max(torch.sqrt(power_matmul(e, N, H, W)), m64), d_max(torch.sqrt(power_fft(e, N, H, W)), m64)))
        for p in (p64, power_fft(c.double(), N, H, W)):
            low += int((p < 10.0 * CLAMP).sum())
            count += p.numel()
    return {"c": c, "e": e, "loss": l64, "grad": g64, "mags": mags,
            "d_loss": max(d_loss(l_r, l64), d_loss(l_f, l64)), "d_grad": max(d_max(g_r, g64), d_max(g_f, g64)), "d_mag": d_mag,
            "low_share": low / count}


def bars(ref):
    """loss: 4 d_ref + 2^-23 (the one rounding of the double result to float); gradient and magnitudes: 4 d_ref."""
    return 4.0 * ref["d_loss"] + 2.0 ** -23, 4.0 * ref["d_grad"], [4.0 * d for d in ref["d_mag"]]
