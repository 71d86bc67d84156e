"""TEST INFRASTRUCTURE: the float64 numpy oracle of chunked enhancement with overlap (include/wunet_hip.h: wunet_chunk_gather,
wunet_chunk_overlap_add).  It restates the geometry and takes the model's chunk outputs as given:

  L = sample_length, m = margin, f = fade, H = L - 2 m - f (the hop), H >= 1 and f <= H.
  A recording of T >= 1 samples has n = max(1, ceil((T - f) / H)) chunks; chunk k reads samples [k H - m, k H - m + L), zeros outside
  [0, T).  For t in [0, T), k = min(t // H, n - 1), j = t - k H, y_k = the model's output for chunk k:
      k >= 1 and j < f:  out[t] = ramp[j] y_k[m + j] + (1 - ramp[j]) y_(k-1)[m + H + j]
      otherwise:         out[t] = y_k[m + j]
  ramp: float32 [f] made in float64 and rounded once - "linear" (j + 0.5) / f, "hann" sin^2(pi (j + 0.5) / (2 f)); 1 - ramp[j] is the
  float32 difference.  The sums and products below are float64 of those float32 values."""
import numpy as np


def hop(L, m, f):
    H = L - 2 * m - f
    assert m >= 0 and f >= 0 and H >= 1 and f <= H, (L, m, f)
    return H


def count(T, L, m, f):
    H = hop(L, m, f)
    return max(1, -(-(T - f) // H))


def ramp(f, window):
    j = np.arange(f, dtype=np.float64)
    if window == "linear":
        r = (j + 0.5) / f
    elif window == "hann":
        r = np.sin(np.pi * (j + 0.5) / (2.0 * f)) ** 2
    else:
        raise AssertionError(window)
    return r.astype(np.float32)


def gather(x, L, m, f):
    """x float32 [T] -> the chunks float32 [n, L]."""
    T, H = len(x), hop(L, m, f)
    out = np.zeros((count(T, L, m, f), L), np.float32)
    for k in range(out.shape[0]):
        for j in range(L):
            t = k * H - m + j
            if 0 <= t < T:
                out[k, j] = x[t]
    return out


def overlap_add(y, T, L, m, f, ramp32):
    """y float32 [n, L], the model's outputs.  Returns out float64 [T]; faded bool [T]; copy float32 [T] = y_k[m + j] (what a sample
    outside the cross-fades must equal bit for bit); wa, wb float64 [T] = |w y_k[m + j]|, |w' y_(k-1)[m + H + j]| inside them."""
    H, n = hop(L, m, f), count(T, L, m, f)
    assert y.shape == (n, L) and y.dtype == np.float32 and (f == 0 or (ramp32.dtype == np.float32 and ramp32.shape == (f,)))
    out, faded, copy = np.zeros(T), np.zeros(T, bool), np.zeros(T, np.float32)
    wa, wb = np.zeros(T), np.zeros(T)
    for t in range(T):
        k = min(t // H, n - 1)
        j = t - k * H
        copy[t] = y[k, m + j]
        if k >= 1 and j < f:
            w = ramp32[j]
            q = np.float32(1.0) - w                       # float32
            assert q.dtype == np.float32
            a, b = float(w) * float(y[k, m + j]), float(q) * float(y[k - 1, m + H + j])
            out[t], faded[t], wa[t], wb[t] = a + b, True, abs(a), abs(b)
        else:
            out[t] = float(copy[t])
    return {"out": out, "faded": faded, "copy": copy, "wa": wa, "wb": wb}


def overlap_add_fast(y, T, L, m, f, ramp32):
    """overlap_add with array indexing, for the real-size rows (tests/chunks_cases.py checks that the two agree on the small cases)."""
    H, n = hop(L, m, f), count(T, L, m, f)
    t = np.arange(T)
    k = np.minimum(t // H, n - 1)
    j = t - k * H
    copy = y[k, m + j]
    faded = (k >= 1) & (j < f)
    out, wa, wb = copy.astype(np.float64), np.zeros(T), np.zeros(T)
    if f:
        kk, jj = k[faded], j[faded]
        w = ramp32[jj]
        q = (np.float32(1.0) - w).astype(np.float32)
        a, b = w.astype(np.float64) * y[kk, m + jj].astype(np.float64), q.astype(np.float64) * y[kk - 1, m + H + jj].astype(np.float64)
        out[faded], wa[faded], wb[faded] = a + b, np.abs(a), np.abs(b)
    return {"out": out, "faded": faded, "copy": copy, "wa": wa, "wb": wb}
