"""Yardsticks of the STOI loss tests (tests/test_stoi_loss_ref.py, tests/test_stoi_loss_emu.py, tests/test_gpu_stoi_loss.py).  No test
functions.  The graph of stoi_ref._one64 restated in torch ops so that autograd gives d loss / d estimate, loss = -mean over the rows
of STOI: the direct polyphase sum, frames, the mask from the clean signal alone (a constant), overlap-add by index_add, the spectrum,
band sums, segments.  Three computations, all on the CPU:
  (i)   oracle64_grad  float64, torch.fft;
  (ii)  float32, torch.fft in float32;
  (iii) float32, the frames times stoi_ref.basis32() by matmul.
The kernels are never compared with (ii) or (iii): those two say how far float32 arithmetic lands from (i) on the same inputs,
d_ref = max over the rows that score and over both of max_t |g32 - g64| / max_t |g64|, and the kernels' bar is 4 d_ref per row.
A row with fewer than 30 spectral frames contributes the constant 1e-5 and a zero gradient."""
import functools

import numpy as np
import torch

import stoi_ref as R


def _resample(x, fs):
    """stoi_ref.resample_direct on a torch vector, differentiable."""
    if fs == R.FS:
        return x
    p, q, L, h = R.taps(fs)
    h = torch.from_numpy(h).to(x.dtype)
    T = len(x)
    n_out = -(-T * p // q)
    c = np.arange(n_out, dtype=np.int64) * q + L
    ihi, ph = c // p, c % p
    y = torch.zeros(n_out, dtype=x.dtype)
    for j in range(2 * L // p + 1):
        tap, i = ph + p * j, ihi - j
        ok = (tap <= 2 * L) & (i >= 0) & (i < T)
        y = y.index_add(0, torch.from_numpy(np.nonzero(ok)[0]), h[torch.from_numpy(tap[ok])] * x[torch.from_numpy(i[ok])])
    return p * y


def _frame_index(n):
    starts = np.array(list(R.frame_starts(n)), dtype=np.int64)
    return torch.from_numpy(starts[:, None] + np.arange(R.N_FRAME, dtype=np.int64)[None, :])


def _bands(power):
    return torch.stack([torch.sqrt(power[:, a:b].sum(dim=1)) for a, b in R.band_edges()], dim=1)


def _row(x, y, fs, dtype, spectrum, detail=None):
    """STOI of one row as a torch scalar of `dtype` (differentiable in y), and the spectral frame count.  detail: a dict that receives
    alpha Y, clip X of every (segment, frame, band)."""
    x, y = _resample(x.to(dtype), fs), _resample(y.to(dtype), fs)
    if len(x) <= R.N_FRAME:
        return None, 0
    w = torch.from_numpy(R.WINDOW).to(dtype)
    idx = _frame_index(len(x))
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
    idx = _frame_index(len(xo))
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
    X, Y = _bands(PX), _bands(PY)
    seg = torch.arange(F - R.SEG + 1)[:, None] + torch.arange(R.SEG)[None, :]
    xs, ys = X[seg], Y[seg]                                             # [segments, 30, 15]
    clip = torch.tensor(R.CLIP, dtype=dtype)
    nx, ny = torch.sqrt((xs * xs).sum(dim=1, keepdim=True)), torch.sqrt((ys * ys).sum(dim=1, keepdim=True))
    ay, cx = ys * (nx / (ny + eps)), xs * clip
    if detail is not None:
        detail["ay"], detail["cx"] = ay.detach(), cx.detach()
    yp = torch.minimum(ay, cx)
    xs = xs - xs.mean(dim=1, keepdim=True)
    yp = yp - yp.mean(dim=1, keepdim=True)
    xs = xs / (torch.sqrt((xs * xs).sum(dim=1, keepdim=True)) + eps)
    yp = yp / (torch.sqrt((yp * yp).sum(dim=1, keepdim=True)) + eps)
    return (xs * yp).sum(dim=1).mean(), F


def loss_and_grad(clean, estimate, fs, dtype=torch.float64, spectrum="fft"):
    """(loss, scores [rows], d loss / d estimate [rows, T]) as float64 numpy, computed in `dtype`: loss = -mean of the rows' STOI, a
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


def kink_margin(clean, estimate, fs):
    """(the least |alpha y - clip x| / (clip x) over all (segment, frame, band) items of all rows, the share of clipped items) in
    float64: how far the inputs are from the kink of min(alpha y, clip x), where the derivative jumps."""
    c = torch.as_tensor(clean).reshape(-1, clean.shape[-1]).double()
    e = torch.as_tensor(estimate).reshape(-1, estimate.shape[-1]).double()
    least, clipped, items = float("inf"), 0, 0
    for r in range(c.shape[0]):
        d = {}
        s, _ = _row(c[r], e[r], fs, torch.float64, "fft", d)
        if s is None:
            continue
        least = min(least, float(((d["ay"] - d["cx"]).abs() / d["cx"]).min()))
        clipped += int((d["ay"] >= d["cx"]).sum())
        items += d["ay"].numel()
    return least, (clipped / items if items else 0.0)


@functools.lru_cache(maxsize=None)
def case_reference(rows, T, fs, gap_len=None):
    """Everything the tests of one case share, computed once and left unchanged: stoi_ref.case_reference plus the float64 loss and
    gradient, d_ref of the gradient, the kink margin and the share of clipped items."""
    ref = dict(R.case_reference(rows, T, fs, gap_len))
    loss, scores, g64 = oracle64_grad(ref["c"], ref["e"], fs)
    scoring = [r for r in range(rows) if ref["frames"][r] >= R.SEG]
    d = {}
    for name, spectrum in (("fft", "fft"), ("matmul", "matmul")):
        g32 = loss_and_grad(ref["c"], ref["e"], fs, torch.float32, spectrum)[2]
        d[name] = max((np.abs(g32[r] - g64[r]).max() / np.abs(g64[r]).max() for r in scoring), default=0.0)
    margin, share = kink_margin(ref["c"], ref["e"], fs) if scoring else (float("inf"), 0.0)
    ref.update({"loss": loss, "scores64": scores, "g64": g64, "scoring": scoring, "dg_fft": float(d["fft"]), "dg_matmul": float(d["matmul"]),
                "dg_ref": float(max(d.values())), "kink": margin, "clipped": share})
    return ref
