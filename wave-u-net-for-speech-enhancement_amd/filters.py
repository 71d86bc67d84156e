"""Recursive (IIR) filters on the device: cascades of second-order sections (include/wunet_hip.h: wunet_sos_windows).

sosfilt(x, sos)            scipy.signal.sosfilt(sos, x) for a batch of rows that stays on its device - a DC blocker, pre-emphasis,
                           a band limit (scipy.signal.butter(..., output="sos") makes the table)
random_biquads(rows, ...)  RNNoise's random spectral shaping: per row a short cascade of random, always stable sections
                           (waveform_dataset.MixLoader(eq_speech=..., eq_noise=...) draws them per batch)
There is no host implementation: CPU tensors need an injected engine (the tests' emulator)."""
import numpy as np
import torch

from . import _lib

MAX_SECTIONS = _lib.CONSTANTS["WUNET_SOS_MAX_SECTIONS"]
MAX_ROWS = 65535                     # rows of one call


def normalise_sos(sos, rows=None):
    """scipy's [S, 6] (one cascade for every row) or [rows, S, 6] table (numpy or tensor; a tensor is brought to the host: the table
    is small and is checked there) -> float32 numpy [S, 5] or [rows, S, 5]: (b0, b1, b2, a1, a2), each section divided by its a0 in
    double and then rounded once.  ValueError for a wrong shape, more than MAX_SECTIONS sections, a0 == 0, a non-finite value or a
    section outside the stability triangle |a2| < 1, |a1| < 1 + a2 (judged on the rounded values, the ones the device runs)."""
    t = sos.detach().cpu().numpy() if isinstance(sos, torch.Tensor) else np.asarray(sos)
    t = np.asarray(t, np.float64)
    if t.ndim not in (2, 3) or t.shape[-1] != 6 or t.shape[-2] < 1:
        raise ValueError(f"sos must have the shape [S, 6] or [rows, S, 6], got {tuple(t.shape)}")
    if t.shape[-2] > MAX_SECTIONS:
        raise ValueError(f"at most {MAX_SECTIONS} sections per cascade, got {t.shape[-2]}")
    if rows is not None and t.ndim == 3 and t.shape[0] != rows:
        raise ValueError(f"sos has {t.shape[0]} cascades for {rows} rows")
    if not np.isfinite(t).all():
        raise ValueError("sos holds a non-finite value")
    if (t[..., 3] == 0.0).any():
        raise ValueError("sos holds a section with a0 == 0")
    k = (t[..., [0, 1, 2, 4, 5]] / t[..., 3:4]).astype(np.float32)
    if not np.isfinite(k).all():
        raise ValueError("sos holds a section whose normalised coefficients overflow float32")
    a1, a2 = k[..., 3].astype(np.float64), k[..., 4].astype(np.float64)
    if not ((np.abs(a2) < 1.0) & (np.abs(a1) < 1.0 + a2)).all():
        raise ValueError("sos holds an unstable section (outside |a2| < 1, |a1| < 1 + a2)")
    return np.ascontiguousarray(k)


def sosfilt(x, sos, engine=None):
    """scipy.signal.sosfilt(sos, x) along the last axis of the float32 tensor x [..., T], every row from rest, on x's device.
    sos: [S, 6] shared by all rows or [rows, S, 6] (rows = x.numel() // T, in x's row order), numpy or tensor, S <= 8; see
    normalise_sos for what is refused.  The coefficients run as float32, state and arithmetic are double, each output is rounded to
    float32 once.  Neither x nor the result is read back to the host."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise ValueError("sosfilt: x must be a float32 tensor")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"sosfilt: needs at least one row of at least one sample, got {tuple(x.shape)}")
    T = x.shape[-1]
    n = x.numel() // T
    k = normalise_sos(sos, n)
    if engine is None:
        from .engine import default_engine
        engine = default_engine()
    flat = x.contiguous().view(-1)
    out = torch.empty(n, 1, T, dtype=torch.float32, device=x.device)
    k = torch.from_numpy(k)
    start = torch.arange(n, dtype=torch.int64) * T
    table = torch.stack([start, start, torch.zeros_like(start), torch.zeros_like(start)], dim=1)
    for r0 in range(0, n, MAX_ROWS):
        r1 = min(n, r0 + MAX_ROWS)
        kk = k[r0:r1] if k.dim() == 3 else k.unsqueeze(0).expand(r1 - r0, -1, -1)
        engine.sos_windows(flat, table[r0:r1].contiguous().to(x.device, non_blocking=True), kk.contiguous().to(x.device, non_blocking=True),
                           out[r0:r1], lead=0)
    return out.view(x.shape)


def random_biquads(rows, sections=2, spread=0.375, p=1.0, generator=None):
    """float32 [rows, sections, 6] in scipy's layout: per section b0 = a0 = 1 and b1, b2, a1, a2 independent, uniform in
    [-spread, spread] - RNNoise's recipe (spread 3/8) for random spectral shaping.  spread < 0.5 keeps every draw inside the stability
    triangle (|a1| < 0.5 < 1 + a2); larger values are refused.  With probability 1 - p a row is the identity in every section.
    The draws, all float64 from `generator`, in this order: torch.rand(rows) - row r passes through the filter when its value is < p -
    then torch.rand(rows, sections, 4), row-major, each value u giving (2 u - 1) spread for b1, b2, a1, a2 in turn.  Both are always
    drawn, whatever p is."""
    rows, sections = int(rows), int(sections)
    if rows < 1 or not 1 <= sections <= MAX_SECTIONS:
        raise ValueError(f"random_biquads: rows >= 1 and 1 <= sections <= {MAX_SECTIONS} expected, got {rows}, {sections}")
    if not 0.0 <= float(spread) < 0.5:
        raise ValueError(f"random_biquads: spread must be in [0, 0.5) for every draw to be stable, got {spread}")
    if not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"random_biquads: p must be in [0, 1], got {p}")
    on = torch.rand(rows, generator=generator, dtype=torch.float64) < float(p)
    u = torch.rand(rows, sections, 4, generator=generator, dtype=torch.float64)
    v = (2.0 * u - 1.0) * float(spread)
    v = torch.where(on[:, None, None], v, torch.zeros_like(v))
    sos = torch.zeros(rows, sections, 6, dtype=torch.float64)
    sos[..., 0] = 1.0
    sos[..., 3] = 1.0
    sos[..., 1:3] = v[..., 0:2]
    sos[..., 4:6] = v[..., 2:4]
    return sos.float()


def sos_to_coefs(sos):
    """random_biquads' (or any a0 == 1) float32 [rows, S, 6] table -> the device's [rows, S, 5] (b0, b1, b2, a1, a2)."""
    return sos[..., [0, 1, 2, 4, 5]].contiguous()
