"""Yardsticks of the ESTOI tests (tests/test_estoi_ref.py, tests/test_estoi_emu.py, tests/test_estoi_loss_emu.py, tests/test_gpu_estoi.py).
No test functions.  The definition is Jensen & Taal 2016 with pystoi's choices for stoi(x, y, fs, extended=True), x = clean, y = estimate,
per row.  Everything up to the band magnitudes is tests/stoi_ref.py (the score) and tests/stoi_loss_ref.py (the loss) - the resamplers,
the removal of silent frames, the spectra, the band sums are imported from there - and only the segment step is stated here: every
segment's 30 x 15 block of X and, separately, of Y is normalised per band over its 30 frames (minus the mean, over the 2-norm + EPS) and
then per frame over its 15 bands (the same), d_m = (1 / 30) sum x~ y~, the score is the mean of d_m.  pystoi adds EPS * randn to the
block before each normalisation; nothing is added here and EPS stands in the denominators (1e-15 on a non-degenerate input; the bar
against pystoi in tests/test_estoi_ref.py, 1e-9, absorbs it).
The score, in numpy, mirrors stoi_ref:
  (i)   oracle64    float64: scipy.signal.resample_poly, np.fft.rfft;
  (ii)  restate32   float32: the direct polyphase sum, frames times the float32 basis by matmul;
  (iii) fft32       float32: scipy's resampler, torch.fft in float32.
The loss and its gradient, in torch autograd, mirror stoi_loss_ref (the direct polyphase sum in all three, because autograd has to pass it):
  (i)   oracle64_grad  float64, torch.fft;   (ii) float32, torch.fft;   (iii) float32, the basis matmul.
The kernels are never compared with (ii) or (iii): those say how far float32 arithmetic lands from (i) on the same inputs (d_ref), and
the kernels' bars are 4 d_ref + 2^-23 (score, loss) and 4 d_ref of a row's largest entry (gradient)."""
import functools

import numpy as np
import torch

import stoi_loss_ref as L
import stoi_ref as R


def _normalise(a, axis):
    """Minus the mean along `axis`, over (the 2-norm along it + EPS), in the dtype of a."""
    dt = a.dtype
    a = a - a.mean(axis=axis, keepdims=True, dtype=dt)
    return a / (np.sqrt((a * a).sum(axis=axis, keepdims=True, dtype=dt)) + dt.type(R.EPS))


def _blocks(X):
    F = X.shape[0]
    return X[np.arange(F - R.SEG + 1)[:, None] + np.arange(R.SEG)[None, :]]          # [segments, 30, 15]


def segments_score(X, Y):
    """The segment step on band magnitudes X, Y [frames, 15] in their dtype; fewer than 30 frames: 1e-5."""
    dt = X.dtype
    if X.shape[0] < R.SEG:
        return R.SHORT
    xs, ys = _normalise(_normalise(_blocks(X), 1), 2), _normalise(_normalise(_blocks(Y), 1), 2)
    return float(((xs * ys).sum(axis=(1, 2), dtype=dt) / dt.type(R.SEG)).mean(dtype=dt))


def least_norms(X, Y):
    """(least centred band-row norm, least centred frame-column norm) over all segments of X and of Y, float64."""
    rows, cols = float("inf"), float("inf")
    if X.shape[0] < R.SEG:
        return rows, cols
    for Z in (X, Y):
        b = _blocks(Z)
        c = b - b.mean(axis=1, keepdims=True)
        rows = min(rows, float(np.sqrt((c * c).sum(axis=1)).min()))
        n = _normalise(b, 1)
        c = n - n.mean(axis=2, keepdims=True)
        cols = min(cols, float(np.sqrt((c * c).sum(axis=2)).min()))
    return rows, cols


def _bands64(x, y, fs):
    """Band magnitudes [frames, 15] of both signals on stoi_ref's float64 path, or None without a frame."""
    x, y = R.resample_scipy(np.asarray(x, np.float64), fs), R.resample_scipy(np.asarray(y, np.float64), fs)
    xo, yo, _ = R.remove_silent(x, y)
    fx, fy = R._frames(xo, R.WINDOW), R._frames(yo, R.WINDOW)
    if len(fx) == 0:
        return None
    return R._bands(np.abs(np.fft.rfft(fx, R.NFFT, axis=1)) ** 2), R._bands(np.abs(np.fft.rfft(fy, R.NFFT, axis=1)) ** 2)


def _one64(x, y, fs):
    b = _bands64(x, y, fs)
    return (R.SHORT, 0) if b is None else (segments_score(*b), len(b[0]))


def _one_restate32(x, y, fs):
    x, y = R.resample_direct(np.asarray(x, np.float64), fs, np.float32), R.resample_direct(np.asarray(y, np.float64), fs, np.float32)
    xo, yo, _ = R.remove_silent(x, y, R.WINDOW.astype(np.float32))
    fx, fy = R._frames(xo, np.ones(R.N_FRAME, np.float32)), R._frames(yo, np.ones(R.N_FRAME, np.float32))   # (the basis carries the window)
    if len(fx) == 0:
        return R.SHORT
    bc, bs = R.basis32()
    return segments_score(R._bands(np.matmul(fx, bc) ** 2 + np.matmul(fx, bs) ** 2), R._bands(np.matmul(fy, bc) ** 2 + np.matmul(fy, bs) ** 2))


def _one_fft32(x, y, fs):
    x, y = R.resample_scipy(np.asarray(x, np.float32), fs).astype(np.float32), R.resample_scipy(np.asarray(y, np.float32), fs).astype(np.float32)
    w32 = R.WINDOW.astype(np.float32)
    xo, yo, _ = R.remove_silent(x, y, w32)
    fx, fy = R._frames(xo, w32), R._frames(yo, w32)
    if len(fx) == 0:
        return R.SHORT
    FX, FY = torch.fft.rfft(torch.from_numpy(fx), R.NFFT, dim=1), torch.fft.rfft(torch.from_numpy(fy), R.NFFT, dim=1)
    return segments_score(R._bands((FX.real ** 2 + FX.imag ** 2).numpy()), R._bands((FY.real ** 2 + FY.imag ** 2).numpy()))


def oracle64(clean, estimate, fs):
    """(scores float64 [rows], spectral frame counts int [rows]) of float32 / float64 tensors or arrays [..., T]."""
    c, e = R._rows(clean), R._rows(estimate)
    res = [_one64(c[r], e[r], fs) for r in range(len(c))]
    return np.array([s for s, _ in res], np.float64), np.array([f for _, f in res], np.int64)


def restate32(clean, estimate, fs):
    c, e = R._rows(clean), R._rows(estimate)
    return np.array([_one_restate32(c[r], e[r], fs) for r in range(len(c))], np.float64)


def fft32(clean, estimate, fs):
    c, e = R._rows(clean), R._rows(estimate)
    return np.array([_one_fft32(c[r], e[r], fs) for r in range(len(c))], np.float64)


def bar(ref):
    """4 d_ref + 2^-23, as stoi_ref.bar."""
    return 4.0 * ref["d_ref"] + 2.0 ** -23


# ------------------------------------------------------------------------------------------------ the loss: torch autograd
def _tnormalise(a, dim, eps):
    a = a - a.mean(dim=dim, keepdim=True)
    return a / (torch.sqrt((a * a).sum(dim=dim, keepdim=True)) + eps)


def _row(x, y, fs, dtype, spectrum):
    """ESTOI of one row as a torch scalar of `dtype` (differentiable in y), and the spectral frame count: stoi_loss_ref._row with the
    segment step replaced (its resampler, frame index and band sums are used as they are)."""
    x, y = L._resample(x.to(dtype), fs), L._resample(y.to(dtype), fs)
    if len(x) <= R.N_FRAME:
        return None, 0
    w = torch.from_numpy(R.WINDOW).to(dtype)
    idx = L._frame_index(len(x))
    xf, yf = w * x[idx], w * y[idx]
    eps = torch.tensor(R.EPS, dtype=dtype)
    en = 20.0 * torch.log10(torch.sqrt((xf * xf).sum(dim=1)) + eps)
    keep = torch.nonzero(en > en.max() - R.DYN_RANGE)[:, 0]              # (the clean signal alone: no gradient flows through it)
    n = len(keep)
    at = (torch.arange(n)[:, None] * R.HOP + torch.arange(R.N_FRAME)[None, :]).reshape(-1)
    xo = torch.zeros((n - 1) * R.HOP + R.N_FRAME, dtype=dtype).index_add(0, at, xf[keep].reshape(-1))
    yo = torch.zeros((n - 1) * R.HOP + R.N_FRAME, dtype=dtype).index_add(0, at, yf[keep].reshape(-1))
    if len(xo) <= R.N_FRAME:
        return None, 0
    idx = L._frame_index(len(xo))
    F = idx.shape[0]
    if F < R.SEG:
        return None, F
    if spectrum == "fft":
        FX, FY = torch.fft.rfft(w * xo[idx], R.NFFT, dim=1), torch.fft.rfft(w * yo[idx], R.NFFT, dim=1)
        PX, PY = FX.real ** 2 + FX.imag ** 2, FY.real ** 2 + FY.imag ** 2
    else:
        bc, bs = (torch.from_numpy(b) for b in R.basis32())
        PX = (xo[idx] @ bc) ** 2 + (xo[idx] @ bs) ** 2
        PY = (yo[idx] @ bc) ** 2 + (yo[idx] @ bs) ** 2
    X, Y = L._bands(PX), L._bands(PY)
    seg = torch.arange(F - R.SEG + 1)[:, None] + torch.arange(R.SEG)[None, :]
    xs, ys = _tnormalise(_tnormalise(X[seg], 1, eps), 2, eps), _tnormalise(_tnormalise(Y[seg], 1, eps), 2, eps)
    return ((xs * ys).sum(dim=(1, 2)) / R.SEG).mean(), F


def loss_and_grad(clean, estimate, fs, dtype=torch.float64, spectrum="fft"):
    """(loss, scores [rows], d loss / d estimate [rows, T]) as float64 numpy, computed in `dtype`: loss = -mean of the rows' ESTOI, a
    short row being the constant 1e-5."""
    c = torch.as_tensor(clean).detach().reshape(-1, clean.shape[-1]).to(dtype)
    e = torch.as_tensor(estimate).detach().reshape(-1, estimate.shape[-1]).to(dtype).clone().requires_grad_(True)
    scores = []
    for r in range(c.shape[0]):
        s, _ = _row(c[r], e[r], fs, dtype, spectrum)
        scores.append(s if s is not None else torch.tensor(R.SHORT, dtype=dtype))
    loss = -torch.stack(scores).double().mean()
    g = torch.autograd.grad(loss, e, allow_unused=True)[0] if loss.requires_grad else None
    g = torch.zeros_like(e) if g is None else g
    return float(loss.detach()), np.array([float(s.detach()) for s in scores], np.float64), g.double().numpy()


def oracle64_grad(clean, estimate, fs):
    return loss_and_grad(clean, estimate, fs, torch.float64, "fft")


@functools.lru_cache(maxsize=None)
def case_reference(rows, T, fs, gap_len=None):
    """Everything the score tests of one case share, computed once and left unchanged: stoi_ref.case_reference's inputs, frame counts
    and energy margin; the float64 ESTOI scores, d_ref, and the least centred row and column norms of the float64 path."""
    base = R.case_reference(rows, T, fs, gap_len)
    c, e = base["c"], base["e"]
    s64, frames = oracle64(c, e, fs)
    assert list(frames) == list(base["frames"])
    d_r = float(np.abs(restate32(c, e, fs) - s64).max())
    d_f = float(np.abs(fft32(c, e, fs) - s64).max())
    norms = [least_norms(*b) for b in (_bands64(x, y, fs) for x, y in zip(R._rows(c), R._rows(e))) if b is not None]
    return {"c": c, "e": e, "score": s64, "frames": frames, "d_restate": d_r, "d_fft": d_f, "d_ref": max(d_r, d_f), "margin": base["margin"],
            "row_norm": min((r for r, _ in norms), default=float("inf")), "col_norm": min((k for _, k in norms), default=float("inf"))}


@functools.lru_cache(maxsize=None)
def loss_reference(rows, T, fs, gap_len=None):
    """case_reference plus the float64 loss and gradient and d_ref of the gradient: the maximum over the rows that score and over both
    float32 yardsticks of max_t |g32 - g64| / max_t |g64|."""
    ref = dict(case_reference(rows, T, fs, gap_len))
    loss, scores, g64 = oracle64_grad(ref["c"], ref["e"], fs)
    scoring = [r for r in range(rows) if ref["frames"][r] >= R.SEG]
    d = {}
    for name in ("fft", "matmul"):
        g32 = loss_and_grad(ref["c"], ref["e"], fs, torch.float32, name)[2]
        d[name] = max((np.abs(g32[r] - g64[r]).max() / np.abs(g64[r]).max() for r in scoring), default=0.0)
    ref.update({"loss": loss, "scores64": scores, "g64": g64, "scoring": scoring, "dg_fft": float(d["fft"]), "dg_matmul": float(d["matmul"]),
                "dg_ref": float(max(d.values()))})
    return ref
