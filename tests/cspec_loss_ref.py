"""Yardsticks of the compressed spectral loss tests (tests/test_cspec_loss_emu.py, tests/test_gpu_cspec_loss.py).  No test functions.
Three computations of the same loss, all on the CPU, as in tests/stft_loss_ref.py (whose inputs, basis and distances are reused):
  (i)   oracle64    the definition in float64: torch.stft(center=True, pad_mode="reflect", return_complex=True) under autograd;
  (ii)  restate32   reflect pad, unfold, times the float32 basis with torch.matmul, the same per-bin formulas in float32;
  (iii) fft32       the oracle's own graph in float32 (torch's FFT).
The kernels are never compared with (ii) or (iii): those two only say how far float32 arithmetic lands from (i) on the same inputs,
d_ref = max(d(ii), d(iii)), and the kernels' bars are multiples of d_ref (bars() below).

The definition, per resolution and per bin of clean (c) and enhanced (e):
    P = re^2 + im^2,  Pc = clamp(P, min=clamp),  A = Pc^(compress / 2),  Z = (re + i im) Pc^((compress - 1) / 2)
    L_i = mean [(1 - complex_weight) (A_c - A_e)^2 + complex_weight |Z_c - Z_e|^2],  loss = mean over the resolutions of L_i."""
import functools

import torch

from stft_loss_ref import CLAMP, basis32, d_loss, d_max, pair  # noqa: F401  (pair: the cases' inputs)


def spec_fft(x, N, H, W):
    """(re, im) of torch.stft in x's dtype: [rows, F, bins] each."""
    T = x.shape[-1]
    win = torch.hann_window(W, periodic=True, dtype=x.dtype)
    X = torch.stft(x.reshape(-1, T), N, hop_length=H, win_length=W, window=win, center=True, pad_mode="reflect", return_complex=True)
    return X.real.transpose(1, 2), X.imag.transpose(1, 2)


def spec_matmul(x, N, H, W):
    """The same spectrum as frames x basis in float32."""
    T = x.shape[-1]
    xp = torch.nn.functional.pad(x.reshape(-1, 1, T), (N // 2, N // 2), mode="reflect")[:, 0]
    frames = xp.unfold(-1, N, H)
    bc, bs = basis32(N, W)
    return torch.matmul(frames, bc), torch.matmul(frames, bs)


def compressed(re, im, compress, clamp):
    pc = torch.clamp(re ** 2 + im ** 2, min=clamp)
    f = pc ** ((compress - 1.0) / 2.0)
    return pc ** (compress / 2.0), re * f, im * f


def loss_of(spec, c, e, resolutions, compress=0.3, complex_weight=0.3, clamp=CLAMP):
    total = 0.0
    for N, H, W in resolutions:
        a_c, zr_c, zi_c = compressed(*spec(c, N, H, W), compress, clamp)
        a_e, zr_e, zi_e = compressed(*spec(e, N, H, W), compress, clamp)
        total = total + ((1.0 - complex_weight) * (a_c - a_e) ** 2 + complex_weight * ((zr_c - zr_e) ** 2 + (zi_c - zi_e) ** 2)).mean()
    return total / len(resolutions)


def _with_grad(spec, c, e, resolutions, dtype, **kw):
    x = e.to(dtype).clone().requires_grad_(True)
    loss = loss_of(spec, c.to(dtype), x, resolutions, **kw)
    loss.backward()
    return loss.detach().double(), x.grad.double()


def oracle64(c, e, resolutions, **kw):
    return _with_grad(spec_fft, c, e, resolutions, torch.float64, **kw)


def restate32(c, e, resolutions, **kw):
    return _with_grad(spec_matmul, c, e, resolutions, torch.float32, **kw)


def fft32(c, e, resolutions, **kw):
    return _with_grad(spec_fft, c, e, resolutions, torch.float32, **kw)


@functools.lru_cache(maxsize=None)
def case_reference(rows, T, resolutions, compress, complex_weight):
    """Everything the tests of one (case, compress, complex_weight) share, computed once and left unchanged: inputs, the float64 loss
    and gradient, d_ref of each, and the share of bins of either signal whose float64 power lies below 10 * clamp."""
    c, e = pair(rows, T)
    kw = dict(compress=compress, complex_weight=complex_weight)
    l64, g64 = oracle64(c, e, resolutions, **kw)
    l_r, g_r = restate32(c, e, resolutions, **kw)
    l_f, g_f = fft32(c, e, resolutions, **kw)
    low, count = 0, 0
    for N, H, W in resolutions:
        for x in (c, e):
            re, im = spec_fft(x.double(), N, H, W)
            low += int((re ** 2 + im ** 2 < 10.0 * CLAMP).sum())
            count += re.numel()
    return {"c": c, "e": e, "loss": l64, "grad": g64,
            "d_loss": max(d_loss(l_r, l64), d_loss(l_f, l64)), "d_grad": max(d_max(g_r, g64), d_max(g_f, g64)), "low_share": low / count}


def bars(ref):
    """loss: 4 d_ref + 2^-23 (the one rounding of the double result to float); gradient: 4 d_ref (max-norm relative) - the margins of
    the STFT loss, for the same reason: the kernels do the float32 work of restate32 in another order of sums."""
    return 4.0 * ref["d_loss"] + 2.0 ** -23, 4.0 * ref["d_grad"]
