"""Sample-rate conversion on the device (include/wunet_hip.h: wunet_resample_rows, csrc/wunet_resample.h).

The network runs at one rate (16 kHz in the reference); a reference user brings a corpus to it with librosa on the host.  Here a
waveform changes its rate where it already lies: `resample` for a batch of equal rows, `resample_many` for recordings of any lengths in
one launch.  The filter is scipy.signal.resample_poly's default - a Kaiser (beta = 5) windowed sinc of half-length 10 max(up, down)
with its cutoff at the lower of the two Nyquist frequencies, unit gain at DC, times `up` - designed here in float64 with numpy and
rounded once to float32, so its shape and gain are data for the kernel.  Rate pairs with max(up, down) <= 640 are accepted:
48, 44.1, 32, 24, 22.05, 11.025 and 8 kHz against 16 kHz among them.  There is no CPU fallback and no gradient.
"""
import functools
import math

import numpy as np
import torch

from . import _lib

MAX_RATIO = _lib.CONSTANTS["WUNET_RESAMPLE_MAX_RATIO"]
MAX_TAPS = _lib.CONSTANTS["WUNET_RESAMPLE_MAX_TAPS"]


def _rate(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError(f"resample: {name} must be a positive integer number of Hz (got {v!r})")
    return int(v)


def rate_ratio(rate_in, rate_out):
    """(up, down) = rate_out / rate_in in lowest terms; ValueError for a rate that is not a positive integer or a pair whose filter
    is above the cap of the kernel."""
    rate_in, rate_out = _rate("rate_in", rate_in), _rate("rate_out", rate_out)
    g = math.gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    if max(up, down) > MAX_RATIO:
        raise ValueError(f"resample: {rate_in} -> {rate_out} Hz is {up} / {down} and needs {20 * max(up, down) + 1} filter taps; at most "
                         f"{MAX_TAPS} are supported (max(up, down) <= {MAX_RATIO})")
    return up, down


def design(up, down):
    """The filter in float64, before its one rounding: up h, h = sinc(n / M) / M kaiser(2 L + 1, 5)[n + L] normalised to sum 1, M = max(up, down),
    L = 10 M (scipy.signal.firwin(2 L + 1, 1 / M, window=("kaiser", 5.0)), resample_poly's default)."""
    M = max(up, down)
    L = 10 * M
    n = np.arange(-L, L + 1, dtype=np.float64)
    h = np.sinc(n / M) / M * np.kaiser(2 * L + 1, 5.0)
    return up * (h / h.sum())


@functools.lru_cache(maxsize=64)
def _taps(up, down):
    h = design(up, down).astype(np.float32)
    h.setflags(write=False)
    return h


def resample_taps(rate_in, rate_out):
    """(up, down, h') for rate_in -> rate_out: h' = up h, h the float64 design of this file's header, float32 [20 max(up, down) + 1]
    (read-only, cached per pair)."""
    up, down = rate_ratio(rate_in, rate_out)
    return up, down, _taps(up, down)


def resampled_length(T, rate_in, rate_out):
    """ceil(T up / down): the samples of T samples at the other rate."""
    up, down = rate_ratio(rate_in, rate_out)
    return -((-int(T) * up) // down)


def _engine(engine):
    if engine is not None:
        return engine
    from .engine import default_engine
    return default_engine()


def uniform_rows(n, T_in, T_out):
    """The table of n rows of T_in samples back to back -> n rows of T_out samples back to back: int64 [n, 4]."""
    i = np.arange(n, dtype=np.int64)
    return np.stack([i * T_in, np.full(n, T_in, np.int64), i * T_out, np.full(n, T_out, np.int64)], axis=1)


def ragged_rows(lengths_in, lengths_out):
    """The table of rows of any lengths, back to back in both arrays: (int64 [n, 4], in total, out total)."""
    a, b = np.asarray(lengths_in, np.int64), np.asarray(lengths_out, np.int64)
    sa, sb = np.concatenate([[0], np.cumsum(a)]), np.concatenate([[0], np.cumsum(b)])
    return np.stack([sa[:-1], a, sb[:-1], b], axis=1).astype(np.int64), int(sa[-1]), int(sb[-1])


@torch.no_grad()
def resample(x, rate_in, rate_out, engine=None, length=None):
    """x: float32 [..., T] on the device.  Every row of the last dimension at the other rate: [..., resampled_length(T)].  Equal rates
    return x itself.  One launch; the row table is the only thing that travels from the host.
    length: another number of output samples per row - fewer than resampled_length(T) truncates (the trim of a round trip), more reads
    zeros behind the row."""
    up, down = rate_ratio(rate_in, rate_out)
    if up == down:
        return x
    if x.dtype != torch.float32:
        raise ValueError(f"resample: float32 expected (got {x.dtype})")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"resample: at least one row of at least one sample expected (got {tuple(x.shape)})")
    T = x.shape[-1]
    To = resampled_length(T, rate_in, rate_out) if length is None else int(length)
    if To < 1:
        raise ValueError(f"resample: length must be >= 1 (got {length!r})")
    flat = x.contiguous().view(-1)
    n = flat.numel() // T
    out = torch.empty(n * To, dtype=torch.float32, device=x.device)
    rows = torch.from_numpy(uniform_rows(n, T, To)).to(x.device, non_blocking=True)
    _engine(engine).resample_rows(flat, rows, out, rate_in, rate_out, To)
    return out.view(*x.shape[:-1], To)


@torch.no_grad()
def resample_many(recordings, rate_in, rate_out, engine=None):
    """recordings: float32 [1, 1, T_r] or [T_r] tensors of any lengths on one device.  Returns them at the other rate in the same
    shapes (views of one buffer), from one launch.  Equal rates return the recordings themselves."""
    up, down = rate_ratio(rate_in, rate_out)
    recordings = list(recordings)
    if up == down or not recordings:
        return recordings
    dev = recordings[0].device
    for x in recordings:
        if not (x.dim() == 1 or (x.dim() == 3 and x.shape[0] == 1 and x.shape[1] == 1)):
            raise ValueError("resample_many: every recording must be [1, 1, T] or [T]")
        if x.dtype != torch.float32 or x.device != dev:
            raise ValueError("resample_many: float32 recordings on one device expected")
        if x.shape[-1] < 1:
            raise ValueError("resample_many: a recording needs at least one sample (got 0)")
    lin = [int(x.shape[-1]) for x in recordings]
    lout = [resampled_length(T, rate_in, rate_out) for T in lin]
    table, tin, tout = ragged_rows(lin, lout)
    flat = torch.cat([x.reshape(-1) for x in recordings]) if len(recordings) > 1 else recordings[0].contiguous().view(-1)
    out = torch.empty(tout, dtype=torch.float32, device=dev)
    _engine(engine).resample_rows(flat, torch.from_numpy(table).to(dev, non_blocking=True), out, rate_in, rate_out, max(lout))
    return [out[s:s + T].view(*x.shape[:-1], T) for x, s, T in zip(recordings, table[:, 2].tolist(), lout)]


def outputs_per_block(rate_in, rate_out, engine=None):
    """The outputs one block of resample_rows_kernel owns per trip for that pair (wunet_resample_tile): what the tests put row lengths
    next to."""
    up, down, h = resample_taps(rate_in, rate_out)
    return int(_engine(engine).lib.wunet_resample_tile(up, down, len(h)))
