"""The yardstick of the row losses (tests/test_loss_rows_emu.py, tests/test_gpu_loss_rows.py): the definition of
include/wunet_hip.h's wunet_loss_rows_forward restated in float64 torch, the gradient by autograd.  It is not the reference
project (which has no such loss) and it shares no code with the kernels.  Inputs are float32 tensors, converted exactly.

The bars (the issue's, derived there from the arithmetic: every sum is double, only the outputs are rounded):
  values    |got - ref| <= 2^-22 * max(|ref|, 1)          the loss and every per-row dB
  gradient  per row max|got - ref| <= 1e-5 * max|ref|    a tenth of the project's 1e-4 parity bar
"""
import math

import torch

VALUE_BAR = 2.0 ** -22
GRAD_BAR = 1e-5
K10 = 10.0 / math.log(10.0)


def per_row(kind, clean, enhanced, zero_mean=True, eps=1e-8):
    """float64 [R] dB values of float64 inputs [..., T] (differentiable)."""
    T = clean.shape[-1]
    s = clean.reshape(-1, T)
    e = enhanced.reshape(-1, T)
    if zero_mean:
        s = s - s.mean(dim=1, keepdim=True)
        e = e - e.mean(dim=1, keepdim=True)
    q = (s * s).sum(dim=1)
    if kind == "si_sdr":
        p = (e * s).sum(dim=1)
        r = (e * e).sum(dim=1)
        alpha = p / (q + eps)
        et = alpha * alpha * q
        en = r - 2.0 * alpha * p + alpha * alpha * q
    elif kind == "snr":
        d = e - s
        et = q
        en = (d * d).sum(dim=1)
    else:
        raise ValueError(kind)
    return K10 * torch.log((et + eps) / (en + eps))


def reference(kind, clean, enhanced, zero_mean=True, eps=1e-8, grad_loss=1.0):
    """(loss, per-row dB [R], d(grad_loss * loss) / d enhanced) in float64 for float32 inputs."""
    s = clean.detach().double().cpu()
    e = enhanced.detach().double().cpu().requires_grad_(True)
    v = per_row(kind, s, e, zero_mean, eps)
    loss = -v.mean()
    (g,) = torch.autograd.grad(loss * grad_loss, e)
    return loss.detach(), v.detach(), g


def check_values(what, got_loss, got_rows, ref_loss, ref_rows):
    """Prints the distances in units of the bar, then asserts them."""
    dl = abs(float(got_loss) - float(ref_loss)) / max(abs(float(ref_loss)), 1.0)
    dr = ((got_rows.double().cpu() - ref_rows).abs() / ref_rows.abs().clamp(min=1.0)).max().item() if got_rows is not None else 0.0
    print(f"{what}: loss {dl:.2e}  rows {dr:.2e}  (bar {VALUE_BAR:.2e})")
    assert math.isfinite(float(got_loss)) and dl <= VALUE_BAR, (what, float(got_loss), float(ref_loss))
    assert dr <= VALUE_BAR, (what, dr)
    return max(dl, dr)


def check_grad(what, got, ref):
    """Per row: max|got - ref| <= GRAD_BAR * max|ref| (a row whose reference gradient is all zero must be all zero)."""
    T = ref.shape[-1]
    g = got.detach().double().cpu().reshape(-1, T)
    r = ref.reshape(-1, T)
    assert torch.isfinite(g).all(), what
    scale = r.abs().amax(dim=1)
    dist = (g - r).abs().amax(dim=1)
    rel = (dist / scale.clamp(min=1e-300)).masked_fill(scale == 0, 0.0)
    print(f"{what}: gradient worst row {rel.max().item():.2e} of its largest element (bar {GRAD_BAR:.0e})")
    assert (dist <= GRAD_BAR * scale).all(), (what, rel.max().item())
    return rel.max().item()


LADDER_DB = (-10.0, 0.0, 20.0, 40.0, 60.0, 80.0)


def ladder(T=4096, seed=0):
    """e = 0.7 s + noise at the input SNRs of LADDER_DB, one per row (float32): the SI-SDR of a row is its input SNR - 3.1 dB.
    The gradient bar holds for the rows up to 60 dB; the 80 dB row is there for the values."""
    rows = len(LADDER_DB)
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(rows, 1, T, generator=g)
    n = torch.randn(rows, 1, T, generator=g)
    snr_db = torch.tensor(LADDER_DB).view(rows, 1, 1)
    e = 0.7 * s + n * (10.0 ** (-snr_db / 20.0))
    return s.contiguous(), e.contiguous()


def pair(R, T, seed=0):
    """A signal-like pair [R, 1, T]: e = 0.8 s + 0.3 noise + a small offset (so the centring does something)."""
    g = torch.Generator().manual_seed(seed * 7919 + R * 131 + T)
    s = torch.randn(R, 1, T, generator=g)
    e = 0.8 * s + 0.3 * torch.randn(R, 1, T, generator=g) + 0.05
    return s.contiguous(), e.contiguous()
