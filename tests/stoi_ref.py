"""Yardsticks and inputs of the STOI tests (tests/test_stoi_ref.py, tests/test_stoi_emu.py, tests/test_gpu_stoi.py).  No test functions.
The definition is Taal et al. 2011 with pystoi's choices for stoi(x, y, fs, extended=False); x = clean, y = estimate, per row.  Three
computations of it, all on the CPU:
  (i)   oracle64    the definition in float64: scipy.signal.resample_poly with pystoi's filter, frames, np.fft.rfft, band matrix;
  (ii)  restate32   the kernels' algorithm restated in float32: the direct polyphase sum, frames times a float32-rounded windowed DFT
                    basis with matmul, float32 band sums and segment statistics;
  (iii) fft32       the oracle's own graph on float32 arrays, torch.fft in float32.
The kernels are never compared with (ii) or (iii): those two only say how far float32 arithmetic lands from (i) on the same inputs,
d_ref = max over the rows of a case of |yardstick - oracle64|, and the kernels' bar is 4 d_ref + 2^-23 (bar() below)."""
import functools
import math

import numpy as np
import torch

FS = 10000
N_FRAME = 256
HOP = 128
NFFT = 512
BANDS = 15
SEG = 30
DYN_RANGE = 40.0
EPS = 2.0 ** -52
CLIP = 1.0 + 10.0 ** (15.0 / 20.0)
SHORT = 1e-5
WINDOW = np.hanning(N_FRAME + 2)[1:-1]


def pq(fs):
    g = math.gcd(FS, fs)
    return FS // g, fs // g


@functools.lru_cache(maxsize=None)
def taps(fs):
    """pystoi's resampling filter in float64: (p, q, L, h[2 L + 1])."""
    p, q = pq(fs)
    fc = 1.0 / (2.0 * max(p, q))
    L = int(math.ceil(52.0 / (28.714 * fc / 10.0)))
    t = np.arange(-L, L + 1, dtype=np.float64)
    h = np.kaiser(2 * L + 1, 0.1102 * (60.0 - 8.7)) * (2.0 * p * fc * np.sinc(2.0 * fc * t))
    return p, q, L, h / h.sum()


def resample_scipy(x, fs):
    """Step 1 of the oracle: scipy's polyphase resampler with pystoi's filter (x: [T] float64)."""
    if fs == FS:
        return x
    from scipy.signal import resample_poly
    p, q, _, h = taps(fs)
    return resample_poly(x, p, q, window=h)


def resample_direct(x, fs, dtype=np.float64):
    """y[n] = p sum_t h[t] x[(n q - t) / p] over -L <= t <= L with p | n q - t, zeros outside x - written as that sum, phase by phase,
    in `dtype` (taps rounded to it first)."""
    if fs == FS:
        return x.astype(dtype)
    p, q, L, h = taps(fs)
    h = h.astype(dtype)
    x = x.astype(dtype)
    T = len(x)
    n_out = -(-T * p // q)
    n = np.arange(n_out, dtype=np.int64)
    c = n * q + L
    ihi, ph = c // p, c % p
    y = np.zeros(n_out, dtype)
    for j in range(2 * L // p + 1):
        tap, i = ph + p * j, ihi - j
        ok = (tap <= 2 * L) & (i >= 0) & (i < T)
        y[ok] += h[tap[ok]] * x[i[ok]]
    return (dtype(p) * y).astype(dtype)


def frame_starts(n):
    return range(0, n - N_FRAME, HOP)          # the bound is strict: a frame that would end exactly at the end is dropped (pystoi)


def frame_energies(x):
    """20 log10(|w x_frame| + EPS) of every frame of the (clean, 10 kHz) signal, float64."""
    x = np.asarray(x, np.float64)
    return np.array([20.0 * np.log10(np.linalg.norm(WINDOW * x[i:i + N_FRAME]) + EPS) for i in frame_starts(len(x))])


def remove_silent(x, y, w=WINDOW):
    """Step 2: both signals rebuilt by overlap-add of the windowed frames whose CLEAN energy is above max - 40 dB.  Works in the dtype
    of x; the mask is taken in that dtype too."""
    dt = x.dtype
    w = w.astype(dt)
    starts = list(frame_starts(len(x)))
    if not starts:
        return x[:0], y[:0], 0
    xf = np.stack([w * x[i:i + N_FRAME] for i in starts])
    yf = np.stack([w * y[i:i + N_FRAME] for i in starts])
    en = 20.0 * np.log10(np.sqrt((xf * xf).sum(axis=1, dtype=dt)) + dt.type(EPS))
    keep = en > en.max() - dt.type(DYN_RANGE)
    xf, yf = xf[keep], yf[keep]
    n = len(xf)
    xo, yo = np.zeros((n - 1) * HOP + N_FRAME, dt), np.zeros((n - 1) * HOP + N_FRAME, dt)
    for k in range(n):
        xo[k * HOP:k * HOP + N_FRAME] += xf[k]
        yo[k * HOP:k * HOP + N_FRAME] += yf[k]
    return xo, yo, n


@functools.lru_cache(maxsize=None)
def band_edges():
    """Step 4 from the formula: [(a_i, b_i)] with a_i / b_i the bins nearest 150 * 2^((2 i -+ 1) / 6) Hz."""
    f = np.arange(NFFT // 2 + 1, dtype=np.float64) * FS / NFFT
    out = []
    for i in range(BANDS):
        lo, hi = 150.0 * 2.0 ** ((2 * i - 1) / 6.0), 150.0 * 2.0 ** ((2 * i + 1) / 6.0)
        out.append((int(np.argmin((f - lo) ** 2)), int(np.argmin((f - hi) ** 2))))
    return tuple(out)


def segments_score(X, Y):
    """Step 5 on band magnitudes X, Y [frames, 15] in their dtype; fewer than 30 frames: 1e-5."""
    dt = X.dtype
    F = X.shape[0]
    if F < SEG:
        return SHORT
    eps, clip = dt.type(EPS), dt.type(CLIP)
    idx = np.arange(F - SEG + 1)[:, None] + np.arange(SEG)[None, :]
    xs, ys = X[idx], Y[idx]                                             # [segments, 30, 15]
    nx = np.sqrt((xs * xs).sum(axis=1, keepdims=True, dtype=dt))
    ny = np.sqrt((ys * ys).sum(axis=1, keepdims=True, dtype=dt))
    yp = np.minimum(ys * (nx / (ny + eps)), xs * clip)
    xs = xs - xs.mean(axis=1, keepdims=True, dtype=dt)
    yp = yp - yp.mean(axis=1, keepdims=True, dtype=dt)
    xs = xs / (np.sqrt((xs * xs).sum(axis=1, keepdims=True, dtype=dt)) + eps)
    yp = yp / (np.sqrt((yp * yp).sum(axis=1, keepdims=True, dtype=dt)) + eps)
    return float((xs * yp).sum(axis=1, dtype=dt).mean(dtype=dt))


def _bands(power):
    """[frames, 257] powers -> [frames, 15] magnitudes in the dtype of `power`."""
    dt = power.dtype
    return np.stack([np.sqrt(power[:, a:b].sum(axis=1, dtype=dt)) for a, b in band_edges()], axis=1)


def _frames(x, w):
    starts = list(frame_starts(len(x)))
    if not starts:
        return np.zeros((0, N_FRAME), x.dtype)
    return np.stack([w * x[i:i + N_FRAME] for i in starts])


def _one64(x, y, fs):
    x, y = resample_scipy(np.asarray(x, np.float64), fs), resample_scipy(np.asarray(y, np.float64), fs)
    xo, yo, _ = remove_silent(x, y)
    fx, fy = _frames(xo, WINDOW), _frames(yo, WINDOW)
    if len(fx) == 0:
        return SHORT, 0
    PX, PY = np.abs(np.fft.rfft(fx, NFFT, axis=1)) ** 2, np.abs(np.fft.rfft(fy, NFFT, axis=1)) ** 2
    return segments_score(_bands(PX), _bands(PY)), len(fx)


def oracle64(clean, estimate, fs):
    """(scores float64 [rows], spectral frame counts int [rows]) of float32 / float64 tensors or arrays [..., T]."""
    c, e = _rows(clean), _rows(estimate)
    res = [_one64(c[r], e[r], fs) for r in range(len(c))]
    return np.array([s for s, _ in res], np.float64), np.array([f for _, f in res], np.int64)


def _rows(x):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return a.reshape(-1, a.shape[-1])


@functools.lru_cache(maxsize=None)
def basis32():
    """w[k] cos / -sin(2 pi k b / 512) for k < 256, all 257 bins, computed in float64 and rounded once to float32."""
    k = np.arange(N_FRAME, dtype=np.int64)[:, None]
    b = np.arange(NFFT // 2 + 1, dtype=np.int64)[None, :]
    ph = ((k * b) % NFFT).astype(np.float64) * (2.0 * math.pi / NFFT)
    return (WINDOW[:, None] * np.cos(ph)).astype(np.float32), (-WINDOW[:, None] * np.sin(ph)).astype(np.float32)


def _one_restate32(x, y, fs):
    x, y = resample_direct(np.asarray(x, np.float64), fs, np.float32), resample_direct(np.asarray(y, np.float64), fs, np.float32)
    w32 = WINDOW.astype(np.float32)
    xo, yo, _ = remove_silent(x, y, w32)
    fx, fy = _frames(xo, np.ones(N_FRAME, np.float32)), _frames(yo, np.ones(N_FRAME, np.float32))     # (the basis carries the window)
    if len(fx) == 0:
        return SHORT
    bc, bs = basis32()
    PX = np.matmul(fx, bc) ** 2 + np.matmul(fx, bs) ** 2
    PY = np.matmul(fy, bc) ** 2 + np.matmul(fy, bs) ** 2
    return segments_score(_bands(PX), _bands(PY))


def _one_fft32(x, y, fs):
    x, y = resample_scipy(np.asarray(x, np.float32), fs).astype(np.float32), resample_scipy(np.asarray(y, np.float32), fs).astype(np.float32)
    w32 = WINDOW.astype(np.float32)
    xo, yo, _ = remove_silent(x, y, w32)
    fx, fy = _frames(xo, w32), _frames(yo, w32)
    if len(fx) == 0:
        return SHORT
    FX, FY = torch.fft.rfft(torch.from_numpy(fx), NFFT, dim=1), torch.fft.rfft(torch.from_numpy(fy), NFFT, dim=1)
    PX, PY = (FX.real ** 2 + FX.imag ** 2).numpy(), (FY.real ** 2 + FY.imag ** 2).numpy()
    return segments_score(_bands(PX), _bands(PY))


def restate32(clean, estimate, fs):
    c, e = _rows(clean), _rows(estimate)
    return np.array([_one_restate32(c[r], e[r], fs) for r in range(len(c))], np.float64)


def fft32(clean, estimate, fs):
    c, e = _rows(clean), _rows(estimate)
    return np.array([_one_fft32(c[r], e[r], fs) for r in range(len(c))], np.float64)


def pair(rows, T, fs, gap_len=None):
    """Speech-like rows, drawn per row r from numpy.random.default_rng(0) in float64 and rounded to float32:
    c = 0.08 sum_{k=1..24} env sin(2 pi (110 + 35 r) k t + 0.9 k^2) / k + 0.002 randn, env = 0.55 + 0.45 sin(2 pi (3.1 + 0.7 r) t), with
    the samples [0.30 + 0.12 r, + 0.15) of the length (gap_len[r] instead of 0.15 where given) scaled by 1e-4, so frames really are
    removed; e = 0.8 c + (0.02 + 0.015 r) randn.  Returns float32 tensors [rows, T]."""
    rng = np.random.default_rng(0)
    t = np.arange(T, dtype=np.float64) / fs
    cs, es = [], []
    for r in range(rows):
        env = 0.55 + 0.45 * np.sin(2.0 * np.pi * (3.1 + 0.7 * r) * t)
        c = np.zeros(T)
        for k in range(1, 25):
            c += env * np.sin(2.0 * np.pi * (110.0 + 35.0 * r) * k * t + 0.9 * k * k) / k
        c = 0.08 * c + 0.002 * rng.standard_normal(T)
        glen = 0.15 if gap_len is None else gap_len[r]
        g0 = int((0.30 + 0.12 * r) * T)
        c[g0:g0 + int(glen * T)] *= 1e-4
        e = 0.8 * c + (0.02 + 0.015 * r) * rng.standard_normal(T)
        cs.append(c)
        es.append(e)
    return torch.from_numpy(np.stack(cs).astype(np.float32)), torch.from_numpy(np.stack(es).astype(np.float32))


def energy_margin(clean, fs):
    """The least distance [dB] of any clean frame's energy from its row's threshold max - 40, over the rows, from the float64 path."""
    best = float("inf")
    for row in _rows(clean):
        en = frame_energies(resample_scipy(np.asarray(row, np.float64), fs))
        if len(en):
            best = min(best, float(np.abs(en - (en.max() - DYN_RANGE)).min()))
    return best


@functools.lru_cache(maxsize=None)
def case_reference(rows, T, fs, gap_len=None):
    """Everything the tests of one case share, computed once and left unchanged: inputs, the float64 scores and frame counts, d_ref,
    the energy margin."""
    c, e = pair(rows, T, fs, gap_len)
    s64, frames = oracle64(c, e, fs)
    d_r = float(np.abs(restate32(c, e, fs) - s64).max())
    d_f = float(np.abs(fft32(c, e, fs) - s64).max())
    return {"c": c, "e": e, "score": s64, "frames": frames, "d_restate": d_r, "d_fft": d_f, "d_ref": max(d_r, d_f), "margin": energy_margin(c, fs)}


def bar(ref):
    """4 d_ref + 2^-23: the margin the project gives its STFT kernels over the same kind of yardstick, plus the one rounding of the
    double result to float (absolute: scores are O(1))."""
    return 4.0 * ref["d_ref"] + 2.0 ** -23
